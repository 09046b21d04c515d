"""The arithmetic contract of the reduced-precision pair-array WEIGHT GRADIENT (plain helper module; imported by
test_train_pieces_cpu.py and test_gpu_train_pieces.py).  Operands, tables, the exact value and the abs-sum are conv_bounds'; the piece
rule and the dropped-product constants are conv_pieces'.

gW[k] = sum over the pairs (i, o) of offset k of in[i]^T (x) gout[o]: both operands are activations (gathered rows), both are split
into their first `pieces` bf16 pieces, "ij" = h_i(in) h_j(gout) is kept iff i + j <= pieces + 1 (conv_pieces.KEEP), fp32 accumulation,
fp32 partial sums per work item added in item order.  Two bounds per mode and output element, in units of the abs-sum
S = sum over the pairs |in||gout| (conv_bounds.worst_ratio adds half an ulp of the wanted value and the denormal floor):

  * against the mode's OWN target -- target(): the float64 sum of the kept products of the exact pieces -- what the three-piece kernel
    is held to against the exact value: conv_bounds.WGRAD_C = 2e-5 on every operand kind and PIECE_WGRAD_C = 2e-6 on "piece_aligned"
    (a reduced kernel adds fewer terms per accumulator in the same way, and the partial sums are reduced as before);
  * against the EXACT value: the same dropped-product argument as conv_pieces.C_EXACT, on top of WGRAD_C:
        pieces 2 drops 22 + 13 + 31 <= 2^-15 of S,   pieces 1 drops also 12 + 21 <= 2^-7 of S.
"""
import ctypes
import functools

import numpy as np
import torch

import conv_bounds as cb
import conv_pieces as cp

# every pair-array weight-gradient case of conv_bounds (all nine <MB, NB>, widths past one workgroup tile, the K = 8 swap launches on
# the stride-2 maps, the identity maps), and one output row: fewer than 32 pairs per offset, every step padded, some offsets empty
ONE_ROW = cb._c("wgrad_tl", "wgrad", 40, 1, 27, 32, 32)
WGRAD_CASES = [c for c in cb.CASES if c.family == "wgrad_tl"] + [ONE_ROW]
WGRAD_IDS = [c.id for c in WGRAD_CASES]
C_EXACT = {3: cb.WGRAD_C, 2: 2.0 ** -15 + cb.WGRAD_C, 1: 2.0 ** -7 + cb.WGRAD_C}

assert len(WGRAD_CASES) == len(set(WGRAD_IDS)) and ONE_ROW.id not in cb.CASE_IDS


def c_own(kind):
    """The bound against the mode's own target."""
    return cb.PIECE_WGRAD_C if kind == "piece_aligned" else cb.WGRAD_C


def piece_sum(feats, gout, nbr, keep):
    """float64 [K, cin, cout]: the sum of the products named in `keep` of the exact pieces of both operands."""
    if nbr is None:
        nbr = np.arange(feats.shape[0], dtype=np.int32)[None]
    nbr = np.asarray(nbr)
    pa = [p.double() for p in cb.split3(feats)]
    pg = [p.double() for p in cb.split3(gout)]
    out = torch.zeros((nbr.shape[0], feats.shape[1], gout.shape[1]), dtype=torch.float64)
    for k in range(nbr.shape[0]):
        o = np.nonzero(nbr[k] >= 0)[0]
        if o.shape[0] == 0:
            continue
        rows = nbr[k, o]
        for ij in keep:
            out[k] += pa[int(ij[0]) - 1][rows].t() @ pg[int(ij[1]) - 1][o]
    return out


@functools.lru_cache(maxsize=12)
def _target(n_in, n_out, K, cin, cout, occ, s2, identity, kind, pieces):
    nbr = cb.case_table((n_in, n_out, K, occ, s2, identity))
    feats, _, gout = cb._operands(n_in, n_out, K, cin, cout, occ if K > 1 else 1.0, kind)
    return piece_sum(feats, gout, nbr, cp.KEEP[pieces])


def target(case, kind, pieces):
    """What a weight gradient with `pieces` pieces computes, without its fp32 accumulation: float64 [K, cin, cout] of a RESOLVED
    case (conv_bounds.resolve); shared, never modified."""
    return _target(case.n_in, case.n_out, case.K, case.cin, case.cout, case.occ, case.opt.get("s2"), bool(case.opt.get("identity")),
                   kind, pieces)


def emulate(case, nbr, kind, keep):
    """conv_bounds.split_emulation standing in for the kernel: fp32 accumulation of the products in `keep`, smallest first."""
    feats, _, gout = cb.operands(case, kind)
    return cb.split_emulation(feats, gout, keep, nbr, case.n_in, wgrad=True)


def distance(a, b, bound, kind):
    """Worst |a - b| in units of the own-target bound of `kind`."""
    return cb.worst_ratio(a, b, bound, c_own(kind))[0]


class WgradLaunch(cb.Launch):
    """conv_bounds.Launch whose weight gradient takes the operand-piece count (3: the entry conv_bounds.Launch calls)."""

    def wgrad(self, feats, gout, pieces=3):
        c = self.case
        assert c.family == "wgrad_tl"
        return self.ops.spconv_wgrad_tl(feats, gout, self.tl, c.K, swap=bool(c.opt.get("swap")), pieces=pieces)


def batched_wgrad(entries, device, pieces):
    """conv_bounds.batched_wgrad through osn_spconv_wgrad_tl_partial_pieces: one partial launch per entry with `pieces` pieces, then
    ONE osn_wgrad_tl_reduce_batch -> [gW]."""
    from openscene_amd import ops
    lib = ops._prep(device)
    jobs = (cb.WgradJob * len(entries))()
    partials, out = [], []
    with ops._Dev(device):
        for i, (run, feats, gout) in enumerate(entries):
            c = run.case
            pl = ops.pair_lists(run.tl) if run.tl is not None else None
            gw = torch.full((c.K, c.cin, c.cout), float("nan"), dtype=torch.float32, device=device)
            nbytes = int(ops._cached("osn_spconv_wgrad_tl_ws_bytes", c.K, c.cin, c.cout))
            partial = torch.empty(nbytes, dtype=torch.uint8, device=device)
            ops.check(lib.osn_spconv_wgrad_tl_partial_pieces(ops._p(feats), ops._p(gout), ops._p(pl), int(bool(c.opt.get("swap"))),
                                                             ops._p(gw), feats.shape[0], gout.shape[0], c.K, c.cin, c.cout,
                                                             ops._p(partial), nbytes,
                                                             ctypes.addressof(jobs) + i * ctypes.sizeof(cb.WgradJob),
                                                             ops._stream(device), pieces),
                      "osn_spconv_wgrad_tl_partial_pieces")
            partials.append(partial)
            out.append(gw)
        ops.check(lib.osn_wgrad_tl_reduce_batch(ctypes.addressof(jobs), len(entries), ops._stream(device)), "osn_wgrad_tl_reduce_batch")
    return out
