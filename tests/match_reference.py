"""What the matching tests compare against (openscene_amd.match, csrc/match.hip), restated independently of the library.

A match is judged on the fp16 operand images of both sides (the library's own bits on the device, the stand-in's on the CPU):

    operands_f64    float64 values of given fp16 operand images
    scores          S = a . b  and  A = |a| . |b|  in float64, [L, M]
    reference       the reference order of every row: S descending, position ascending -> (idx [L, k], S of those)
    decided         rows whose reference list is beyond doubt: every adjacent gap among the reference's first k + 1 exceeds
                    C (A_i + A_j), C = conv_bounds.FWD_C -- the project's bound for an fp32-accumulating MFMA contraction
    check           the conditions a result must meet (below); raises AssertionError, returns the worst error / limit
    check_exact     integer inputs: idx and score equal a stable integer argsort bit for bit
    match_chain     a CPU "kernel": fp32 accumulation in ascending d, keys as the contract orders them; with `wrong`, one of the
                    wrong kernels the checker must catch
    vote            ops.knn_vote's rule restated

The conditions of `check`:
    count = min(k, M); idx = -1 and score = -inf past count, 0 <= idx < M before it
    every returned score is within C A of S for the returned pair
    a row's list is strictly descending in key: score descending (-0 as +0), equal scores by ascending position
    on decided rows idx equals the reference's
    on every row the j-th returned score is >= the reference's j-th S minus C A_max of the row
"""
import functools

import torch

import gram_reference as gr
import search_reference as sr
from conv_bounds import FWD_C as C       # the project's bound for an fp32-accumulating MFMA contraction, per abs-sum

K = 8
L_ROWS = 300
MS = (9, 129, 700, 4226)         # M < k + 1 .. one tile and a row .. five tiles and a ragged edge .. many tiles (34), ragged
DIMS_FP16 = (24, 520, 768, 1024)
DIMS_FP8 = (16, 528, 768, 1024)  # an fp8 row is a multiple of 16 wide: 24 and 520 become their fp8 neighbours, as in gram_reference.DIMS
UNDECIDED_MAX = 0.05
PLANT_K = 5                      # label transfer on the planted scenes (tests/test_match_cpu.py establishes the accuracy)
PLANT_ACCURACY = 0.95


def operands_f64(image):
    assert image.dtype == torch.float16
    return image.detach().cpu().double()


def scores(a, b):
    """a float64 [L, d], b float64 [M, d] -> (S, A) float64 [L, M]"""
    return a @ b.t(), a.abs() @ b.abs().t()


def reference(s, k):
    """-> (idx int64 [L, min(k, M)], the S of those): S descending, position ascending (a stable sort)"""
    order = torch.sort(-s, dim=1, stable=True)[1][:, :k]
    return order, torch.gather(s, 1, order)


def decided(s, a, k, c=C):
    """bool [L]: every adjacent gap among the reference's first k + 1 exceeds c (A_i + A_j)"""
    order = torch.sort(-s, dim=1, stable=True)[1][:, :k + 1]
    ss, aa = torch.gather(s, 1, order), torch.gather(a, 1, order)
    if ss.shape[1] < 2:
        return torch.ones(s.shape[0], dtype=torch.bool)
    return ((ss[:, :-1] - ss[:, 1:]) > c * (aa[:, :-1] + aa[:, 1:])).all(dim=1)


def check(idx, score, count, s, a, k, c=C, label=""):
    """The conditions of the module docstring on one result.  -> (worst |score - S| / (c A), share of undecided rows)"""
    idx, score, count = idx.cpu().long(), score.cpu(), count.cpu().long()
    l, m = s.shape
    kk = min(k, m)
    assert idx.shape == (l, k) and score.shape == (l, k) and count.shape == (l,), label
    assert score.dtype == torch.float32, label
    assert bool((count == kk).all()), "%s: count" % label
    assert bool((idx[:, kk:] == -1).all()) and bool((score[:, kk:] == float("-inf")).all()), "%s: padding" % label
    got_i, got_s = idx[:, :kk], score[:, :kk].double()
    assert bool(((got_i >= 0) & (got_i < m)).all()), "%s: a position outside the exemplar list" % label
    want, lim = torch.gather(s, 1, got_i), c * torch.gather(a, 1, got_i)
    err = (got_s - want).abs()
    worst = float((err / lim.clamp(min=1e-300)).max()) if err.numel() else 0.0
    assert bool((err <= lim).all()), "%s: a score beyond c A of its pair (worst %.2f)" % (label, worst)
    if kk > 1:                                               # strictly descending in key
        s0, s1 = got_s[:, :-1] + 0.0, got_s[:, 1:] + 0.0
        assert bool(((s0 > s1) | ((s0 == s1) & (got_i[:, :-1] < got_i[:, 1:]))).all()), "%s: a list not descending in key" % label
    ref_i, ref_s = reference(s, k)
    sure = decided(s, a, k, c)
    assert torch.equal(got_i[sure], ref_i[sure]), "%s: a decided row differs from the reference" % label
    floor = ref_s - c * a.amax(dim=1, keepdim=True)
    assert bool((got_s >= floor).all()), "%s: a returned score below the reference's at its rank" % label
    return worst, 1.0 - float(sure.double().mean())


def check_exact(idx, score, count, xa, xb, k):
    """xa int64 [L, d], xb int64 [M, d], every sum below 2^24: idx and score equal the stable integer argsort bit for bit."""
    s = xa @ xb.t()
    m = s.shape[1]
    kk = min(k, m)
    order = torch.sort(-s, dim=1, stable=True)[1][:, :kk]
    assert torch.equal(idx.cpu().long()[:, :kk], order), "idx differs from the stable integer argsort"
    want = torch.gather(s, 1, order).float()
    assert torch.equal(score.cpu()[:, :kk].view(torch.int32), want.view(torch.int32)), "score bits"   # (+0 for a zero sum, never -0)
    assert bool((idx.cpu()[:, kk:] == -1).all()) and bool((score.cpu()[:, kk:] == float("-inf")).all())
    assert bool((count.cpu() == kk).all())


# ------------------------------------------------------------------------------------------------------ the CPU "kernel"
WRONG = ("ties_to_higher", "last_tile_dropped", "unnormalised", "split_lost", "off_by_one", "fp16_scores")


def chain_f32(a16, b16):
    """float32 [L, M]: the products of the fp16 operands (exact in float32) accumulated one after the other in ascending d"""
    a, b = a16.float(), b16.float()
    acc = torch.zeros(a.shape[0], b.shape[0], dtype=torch.float32)
    for t in range(a.shape[1]):
        acc += a[:, t, None] * b[None, :, t]
    return acc


def match_chain(a16, b16, k, wrong=None, raw_b=None, tile=128, splits=3):
    """-> (idx int32 [L, k], score float32 [L, k], count int32 [L]) of the fp16 operand images a16 [L, d], b16 [M, d]; `wrong`
    names the defect (raw_b: the exemplars left unnormalised, for "unnormalised")."""
    assert wrong is None or wrong in WRONG
    if wrong == "unnormalised":
        b16 = raw_b
    s = chain_f32(a16, b16) + 0.0                           # (-0 as +0)
    l, m = s.shape
    if wrong == "fp16_scores":
        s = s.half().float()
    live = torch.ones(m, dtype=torch.bool)
    if wrong == "last_tile_dropped":
        live[(m - 1) // tile * tile:] = False
        if not bool(live.any()):
            live[:] = True                                   # (a single tile: the defect does not show)
    if wrong == "split_lost":
        n_t = (m + tile - 1) // tile
        per = (n_t + splits - 1) // splits
        live[per * tile:2 * per * tile] = False              # the second part
        if not bool(live.any()):
            live[:] = True
    rank = torch.where(torch.isnan(s), torch.full_like(s, float("-inf")), s)
    rank = torch.where(live[None, :], rank, torch.full_like(rank, float("-inf")))
    if wrong == "ties_to_higher":
        order = (m - 1) - torch.sort(-rank.flip(1), dim=1, stable=True)[1]
    else:
        order = torch.sort(-rank, dim=1, stable=True)[1]
    kk = min(k, int(live.sum()))
    order = order[:, :kk]
    idx = torch.full((l, k), -1, dtype=torch.int32)
    score = torch.full((l, k), float("-inf"), dtype=torch.float32)
    idx[:, :kk] = order.int() + (1 if wrong == "off_by_one" else 0)
    score[:, :kk] = torch.gather(s, 1, order)
    return idx, score, torch.full((l,), min(k, m), dtype=torch.int32)


# ------------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def rows_case(d, m, l=L_ROWS):
    """Seeded Gaussian directions with per-row scales U(0.5, 2), as fp16: (query rows [l, d], exemplar rows [m, d])"""
    gen = torch.Generator().manual_seed(1000 * d + m)
    return sr.unit_rows(l, d, gen).half(), sr.unit_rows(m, d, gen).half()


def operands_cpu(x16, normalize=True):
    """The contract's operand image of fp16 rows, on the CPU (gram_reference's stand-in): fp16 [n, d]"""
    n = x16.shape[0]
    return gr._operands_f16(x16.float(), torch.ones(n), torch.arange(n), normalize)


def integer_case(d, m, l=150, seed=0):
    """Rows of integers |v| <= 8 (every sum is an integer below 2^24), the exemplars with duplicates: many exact ties."""
    gen = torch.Generator().manual_seed(7 * d + m + seed)
    xa = torch.randint(-8, 9, (l, d), generator=gen)
    xb = torch.randint(-8, 9, (m, d), generator=gen)
    if m > 2:
        dup = torch.randint(0, m, (m // 3,), generator=gen)
        xb[torch.randint(0, m, (m // 3,), generator=gen)] = xb[dup].clone()
    xa[::17] = 0                                             # zero rows: every score +0
    return xa, xb


def vote(labels, idx, count, fill=-1):
    """ops.knn_vote restated: the label most of a row's matches hold, ties to the label whose first holder comes first."""
    idx, count = idx.cpu().long(), count.cpu().long()
    out = torch.full((idx.shape[0],), fill, dtype=torch.int64)
    for i in range(idx.shape[0]):
        held = [int(labels[j]) for j in idx[i, :int(count[i])].tolist() if j >= 0 and int(labels[j]) >= 0]
        best, best_n = fill, 0
        for lab in held:                                     # in list order: the first holder of a label wins a tie
            n = held.count(lab)
            if n > best_n:
                best, best_n = lab, n
        out[i] = best
    return out


def planted_reference(a, b, labels, k=PLANT_K):
    """The reference's label transfer in float64 on given operand values: (labels int64 [L], decided bool [L])"""
    s, aa = scores(a, b)
    ref_i, _ = reference(s, k)
    count = torch.full((s.shape[0],), ref_i.shape[1], dtype=torch.int64)
    return vote(labels, ref_i, count), decided(s, aa, k)
