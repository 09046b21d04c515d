"""The arithmetic contract of the reduced-precision convolution modes (plain helper module; imported by test_conv_pieces_cpu.py and
test_gpu_conv_pieces.py).  Everything else -- operands, tables, the exact value, the abs-sum -- is conv_bounds'.

A mode has `pieces` in {3, 2, 1} (csrc/split.h): both operands are split into their first `pieces` bf16 pieces and the product
"ij" = h_i(a) h_j(b) is kept iff i + j <= pieces + 1, accumulated in fp32 smallest first:

    pieces 3  "bf16x6"   31 22 13 21 12 11      (conv_bounds.KEPT: today's kernels)
    pieces 2  "bf16x3"   21 12 11
    pieces 1  "bf16x1"   11

Two bounds per mode, both per output element and in units of the abs-sum  S = sum_k |a_k| |b_k|  (conv_bounds.worst_ratio adds half
an ulp of the wanted value and the denormal floor):

  * against the mode's OWN target -- target(): the float64 sum of the kept products of the exact pieces -- conv_bounds.FWD_C = 2e-6,
    the accumulation budget of the six-product kernels (a reduced kernel adds fewer terms per accumulator in the same way).  This pins
    the arithmetic: a lost product, a wrong plane or an ignored `pieces` lands far outside (figures: test_conv_pieces_cpu.py).

  * against the EXACT value: FWD_C plus the dropped products.  With |h1| <= |x| (1 + 2^-9), |h2| <= 2^-8 |x|, |h3| <= 2^-17 |x|
    (conv_bounds), per term of S and to first order:
        pieces 2 drops 22 + 13 + 31  <=  2^-16 + 2^-17 + 2^-17                 =  2^-15          C2 = 2^-15 + FWD_C
        pieces 1 drops also 12 + 21  <=  2^-8 + 2^-8 (+ the 2^-15 above)       ~  2^-7           C1 = 2^-7  + FWD_C
    (the second-order leftovers -- h1's own 2^-9 excess times 2^-8, the 2^-15 inside C1 -- are below FWD_C's slack: the emulation's
    worst ratio is 0.60 of C2 and 0.992 of C1, the latter on "piece_aligned", which is tight by construction.)
"""
import functools

import torch

import conv_bounds as cb
from oracle import sparse_ops as so

KEEP = {3: ("31", "22", "13", "21", "12", "11"), 2: ("21", "12", "11"), 1: ("11",)}
C_EXACT = {3: cb.FWD_C, 2: 2.0 ** -15 + cb.FWD_C, 1: 2.0 ** -7 + cb.FWD_C}
MODES = {3: "bf16x6", 2: "bf16x3", 1: "bf16x1"}

assert all(set(KEEP[p]) == {ij for ij in cb.KEPT + cb.DISCARDED if int(ij[0]) + int(ij[1]) <= p + 1} for p in KEEP)
assert set(KEEP[3]) == set(cb.KEPT)

# the forward cases of the four families that have reduced instances, as conv_bounds states them
FWD_CASES = [c for c in cb.CASES if c.op == "fwd" and c.family in ("rg", "ws", "tl", "dense")]
FWD_IDS = [c.id for c in FWD_CASES]


def piece_sum(feats, w, nbr, keep):
    """float64 [n_out, cout]: the sum of the products named in `keep` of the exact pieces, through the oracle's convolution."""
    if nbr is None:
        import numpy as np
        nbr = np.arange(feats.shape[0], dtype=np.int32)[None]
    w3 = w if w.dim() == 3 else w.unsqueeze(0)
    pa, pb = cb.split3(feats), cb.split3(w3)
    out = None
    with torch.no_grad():
        for ij in keep:
            t = so.sparse_conv(pa[int(ij[0]) - 1].double(), pb[int(ij[1]) - 1].double(), nbr)
            out = t if out is None else out + t
    return out


@functools.lru_cache(maxsize=12)
def _target(n_in, n_out, K, cin, cout, occ, s2, identity, kind, pieces):
    nbr = cb.case_table((n_in, n_out, K, occ, s2, identity))
    feats, w, _ = cb._operands(n_in, n_out, K, cin, cout, occ if K > 1 else 1.0, kind)
    return piece_sum(feats, w, nbr, KEEP[pieces])


def target(case, kind, pieces):
    """What a launch with `pieces` pieces computes, without its fp32 accumulation: float64 [n_out, cout] of a RESOLVED case
    (conv_bounds.resolve); shared, never modified."""
    return _target(case.n_in, case.n_out, case.K, case.cin, case.cout, case.occ, case.opt.get("s2"), bool(case.opt.get("identity")),
                   kind, pieces)


def distance(a, b, bound):
    """Worst |a - b| in units of FWD_C * abs-sum (+ half an ulp of b + the floor): how far two results sit from each other on the
    scale the first bound is asked on."""
    return cb.worst_ratio(a, b, bound, cb.FWD_C)[0]


class PiecesLaunch(cb.Launch):
    """conv_bounds.Launch whose forward takes the operand-piece count (3: the entry conv_bounds.Launch calls)."""

    def fwd(self, feats, w, pieces=3, bn_partial=None):
        ops, c, o = self.ops, self.case, self.case.opt
        wp = self.image(w)
        if c.family == "rg":
            return ops.spconv_fwd_rg(feats, wp, self.nbr, c.n_out, c.cout, out_rows=self.rows, pieces=pieces)
        if c.family == "ws":
            return ops.spconv_fwd_ws(feats, wp, self.tl, None if o["direct"] else self.nbr, c.n_out, c.K, c.cout,
                                     swap=bool(o["swap"]), direct=bool(o["direct"]), pieces=pieces)
        if c.family == "tl":
            return ops.spconv_fwd_tl(feats, wp, self.tl, c.n_out, c.K, c.cout, bn_partial=bn_partial, pieces=pieces)
        assert c.family == "dense" and ops.dense_eligible(c.cin, c.cout)
        return ops.dense_fwd(feats, wp, c.cout, pieces=pieces)
