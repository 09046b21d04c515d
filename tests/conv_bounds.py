"""The arithmetic contract of the convolutions in one place (plain helper module; imported by test_gpu_fullsize.py,
test_conv_bounds_cpu.py, test_gpu_conv_bounds.py, test_gpu_wgrad_batch.py and the instance census conv_census.py): the bounds, the operand
kinds, the CPU restatements, the CASES, and the Launch that runs a case's kernel on a device.

Contract: every output element lies within  c * sum_k |a_k| |b_k|  of the float64 value, c = 2e-6 for the forward and the input
gradient, 2e-5 for the weight gradient, whatever the dynamic range of the operands; plus half an ulp of the result itself
(6e-8 |want|) and an absolute floor at the denormal edge (1e-37).

Split-bf16 kernels write x = h1 + h2 + h3 (three round-to-nearest bf16 pieces) per operand and keep six of the nine cross products
(KEPT); |h2| <= 2^-8 |x| and |h3| <= 2^-17 |x|, so ONE lost product is at most 2^-16 (h2h2) or 2^-17 (h1h3, h3h1) of |a||b| per term.
Against 2e-6 that shows when the terms are coherent -- the "piece_aligned" operands make them so -- but against the weight gradient's
2e-5 (= 2^-15.6) it cannot: no operand reaches it.  The weight gradient is therefore held to PIECE_WGRAD_C = 2e-6 ON "piece_aligned"
in addition to 2e-5 on every kind: with all-positive operands the only other error is the fp32 accumulation of at most a few thousand
coherent terms, which test_conv_bounds_cpu.py shows to sit far below 2e-6 for the emulation at every shape used here.
"""
import collections
import ctypes
import functools
import zlib

import numpy as np
import torch

from oracle import coords as oc
from oracle import sparse_ops as so
from openscene_amd import synthetic as syn

FWD_C = 2e-6             # forward, input gradient
WGRAD_C = 2e-5           # weight gradient (every kind)
PIECE_WGRAD_C = 2e-6     # weight gradient on "piece_aligned" (see the module docstring)
KINDS = ("row_scales", "cancellation", "gradient_sized", "wide_elements", "piece_aligned")
KEPT = ("11", "12", "21", "13", "31", "22")          # h_i(a) h_j(b) the kernels compute
DISCARDED = ("23", "32", "33")                       # <= 2^-25 |a||b| each
# mantissa of every "piece_aligned" element: h1 = 1, h2 = 2^-8 (the residual 2^-8 - 2^-17 rounds up), h3 = -2^-17
PIECE_MANTISSA = 1.0 + 2.0 ** -8 - 2.0 ** -16 + 2.0 ** -17


def adversarial(kind, n, cin, g):
    if kind == "piece_aligned":        # positive, power-of-two scales over six decades, every element with the same piece ratios
        return 2.0 ** torch.randint(-10, 11, (n, cin), generator=g).float() * PIECE_MANTISSA
    x = torch.randn(n, cin, generator=g)
    if kind == "row_scales":           # per-row magnitudes 1e-6 .. 1e6: a tile mixes huge and tiny rows
        x = x * (10.0 ** (torch.rand(n, 1, generator=g) * 12 - 6))
    elif kind == "cancellation":       # channel pairs (a, -a(1 + 2^-12)): products cancel to ~2^-12 of their size
        p = cin // 2 * 2               # (an odd last channel has no partner)
        x[:, 1:p:2] = -x[:, 0:p:2] * (1 + 2.0 ** -12)
    elif kind == "gradient_sized":     # operands of the size of late-training gradients
        x = x * 1e-8
    elif kind == "wide_elements":      # element-wise magnitudes over 12 decades inside every row
        x = x * (10.0 ** (torch.rand(n, cin, generator=g) * 12 - 6))
    return x


def adversarial_weight(kind, K, cin, cout, g, fan):
    """[K, cin, cout] weights that go with adversarial(kind, ...) features: randn / sqrt(fan), equal weights on the cancelling
    channel pairs, piece-aligned powers of two for "piece_aligned"."""
    if kind == "piece_aligned":
        return 2.0 ** torch.randint(-6, 1, (K, cin, cout), generator=g).float() * PIECE_MANTISSA
    w = torch.randn(K, cin, cout, generator=g) / np.sqrt(fan)
    if kind == "cancellation":
        p = cin // 2 * 2
        w[:, 1:p:2, :] = w[:, 0:p:2, :]
    return w


def worst_ratio(got, want, bound, c):
    """(worst err / lim, number of elements beyond lim): err against the float64 value, lim = c * abs-sum + the fp32 representation
    of the result itself (half an ulp) + an absolute floor at the denormal edge."""
    want = want.detach().double().cpu()
    err = (got.detach().double().cpu() - want).abs()
    lim = c * bound + 6e-8 * want.abs() + 1e-37
    bad = ~(err <= lim)                                   # (a NaN is beyond every bound)
    return float(torch.nan_to_num(err / lim, nan=float("inf")).max()) if err.numel() else 0.0, int(bad.sum())


def within(got, want, bound, c, label):
    ratio, n_bad = worst_ratio(got, want, bound, c)
    assert n_bad == 0, "%s: %d elements beyond the bound, worst ratio %.2f" % (label, n_bad, ratio)
    return ratio


def injective(nbr):
    """Does every input row appear at most once per offset (true of every real kernel map)?"""
    for k in range(nbr.shape[0]):
        v = nbr[k][nbr[k] >= 0]
        if np.unique(v).shape[0] != v.shape[0]:
            return False
    return True


Bounds = collections.namedtuple("Bounds", "out gin gw b_out b_gin b_gw")


def abs_sum_bounds(nbr, feats, w, gout, with_gin=True):
    """float64 forward / input gradient / weight gradient of out[o] = sum_k feats[nbr[k, o]] @ w[k] under `gout`, and the three
    abs-sum bounds (the same operators on |.|), for an int32 [K, n_out] table over feats.shape[0] input rows (None: the identity).
    b_gin goes through oracle.coords.transpose_table, which needs a table that is injective per offset (with_gin=False otherwise)."""
    n_in = feats.shape[0]
    if nbr is None:
        nbr = np.arange(n_in, dtype=np.int32)[None]
    nbr = np.asarray(nbr)
    K = nbr.shape[0]
    w3 = w if w.dim() == 3 else w.unsqueeze(0)
    f64 = feats.double().requires_grad_(True)
    w64 = w3.double().requires_grad_(True)
    ref = so.sparse_conv(f64, w64, nbr)
    ref.backward(gout.double())
    with torch.no_grad():
        fa, ga, wa = feats.double().abs(), gout.double().abs(), w3.double().abs()
        b_out = so.sparse_conv(fa, wa, nbr)
        b_gin = None
        if with_gin:
            assert injective(nbr), "transpose_table needs every input row at most once per offset"
            b_gin = so.sparse_conv(ga, wa.transpose(1, 2).contiguous(), oc.transpose_table(nbr, n_in))
        b_gw = torch.zeros(w3.shape, dtype=torch.float64)
        for k in range(K):
            o = np.nonzero(nbr[k] >= 0)[0]
            b_gw[k] = fa[nbr[k, o]].t() @ ga[o]
    return Bounds(ref.detach(), f64.grad, w64.grad, b_out, b_gin, b_gw)


def split3(x):
    """x = h1 + h2 + h3 exactly: three round-to-nearest bf16 pieces (held as fp32), csrc/split.h."""
    x = x.float()
    h1 = x.bfloat16().float()
    r1 = x - h1
    h2 = r1.bfloat16().float()
    r2 = r1 - h2
    return h1, h2, r2.bfloat16().float()


def split_emulation(a, b, keep, nbr=None, n_in=None, wgrad=False):
    """The split-bf16 contract restated on the CPU: both operands in three bf16 pieces, the cross products named in `keep`
    ("ij" = h_i(a) h_j(b)) accumulated in fp32, smallest products first as the kernels do.
    Forward (wgrad=False): a = features [n_in, cin], b = weights [K, cin, cout] -> [n_out, cout] through the int32 [K, n_out] table
    `nbr` (None: identity).  Weight gradient: a = features, b = output gradient [n_out, cout] -> [K, cin, cout]."""
    n_in = a.shape[0] if n_in is None else int(n_in)
    assert a.shape[0] == n_in
    if nbr is None:
        nbr = np.arange(n_in, dtype=np.int32)[None]
    nbr = torch.as_tensor(np.asarray(nbr)).long()
    assert int(nbr.max()) < n_in
    K, n_out = nbr.shape
    if not wgrad and b.dim() == 2:
        b = b.unsqueeze(0)
    pa, pb = split3(a), split3(b)
    keep = sorted(keep, key=lambda ij: -(int(ij[0]) + int(ij[1])))
    out = torch.zeros((K, a.shape[1], b.shape[1]) if wgrad else (n_out, b.shape[2]), dtype=torch.float32)
    for k in range(K):
        o = torch.nonzero(nbr[k] >= 0).reshape(-1)
        if o.numel() == 0:
            continue
        rows = nbr[k][o]
        ga = [p[rows] for p in pa]
        acc = torch.zeros((a.shape[1], b.shape[1]) if wgrad else (o.numel(), b.shape[2]), dtype=torch.float32)
        for ij in keep:
            i, j = int(ij[0]) - 1, int(ij[1]) - 1
            acc += (ga[i].t() @ pb[j][o]) if wgrad else (ga[i] @ pb[j][k])
        if wgrad:
            out[k] = acc
        else:
            out[o] += acc
    return out


def fmaf_chain_fwd(feats, w, nbr):
    """The stem's small-map forward contract on the CPU: per output element ONE fp32 fused-multiply-add chain over the offsets in
    ascending order, channels ascending inside an offset, an absent neighbour as a zero row (csrc/stem.hip: stem_fwd_kernel).
    fma(x, w, acc) = fp32(x * w + acc) with the product exact in float64."""
    nbr = np.asarray(nbr)
    K, n_out = nbr.shape
    f = feats.numpy().astype(np.float64)
    wd = w.numpy().astype(np.float64)
    acc = np.zeros((n_out, w.shape[2]), dtype=np.float32)
    for k in range(K):
        x = np.where((nbr[k] >= 0)[:, None], f[np.maximum(nbr[k], 0)], 0.0)
        for ci in range(f.shape[1]):
            acc = (x[:, ci, None] * wd[k, ci][None, :] + acc.astype(np.float64)).astype(np.float32)
    return torch.from_numpy(acc)


def fmaf_chain_wgrad(feats, gout, nbr, rows_per_part=64, max_parts=128):
    """The stem's small-map weight gradient on the CPU (stem_wgrad_kernel + stem_wgrad_reduce_kernel): part p chains the rows of the
    64-row chunks p, p + parts, ... in ascending order, the parts are then added in ascending order."""
    nbr = np.asarray(nbr)
    K, n_out = nbr.shape
    f = feats.numpy().astype(np.float64)
    gd = gout.numpy().astype(np.float64)
    n_chunks = -(-n_out // rows_per_part)
    parts = min(n_chunks, max_parts)
    total = None
    for p in range(parts):
        acc = np.zeros((K, f.shape[1], gd.shape[1]), dtype=np.float32)
        for ch in range(p, n_chunks, parts):
            for o in range(ch * rows_per_part, min(n_out, (ch + 1) * rows_per_part)):
                x = np.where((nbr[:, o] >= 0)[:, None], f[np.maximum(nbr[:, o], 0)], 0.0)            # [K, cin]
                acc = (x[:, :, None] * gd[o][None, None, :] + acc.astype(np.float64)).astype(np.float32)
        total = acc if total is None else (total + acc).astype(np.float32)
    return torch.from_numpy(total)


# ---------------------------------------------------------------------------------------------------------------- the cases
# family: the kernel family; op: "fwd" (features x weight image) or "wgrad"; opt: what the entry point is called with (bm: the tile
# height of the case's tile lists where it is not osn_tile_rows' for the row count)
Case = collections.namedtuple("Case", "id family op n_in n_out K cin cout occ opt")
STEM_MFMA_ROWS = 32768 + 17


def _c(family, op, n_in, n_out, K, cin, cout, occ=0.3, **opt):
    tag = "-".join([family, op, "%dx%d" % (n_in, n_out), "k%d" % K, "%dto%d" % (cin, cout)] + ["%s=%s" % kv for kv in sorted(opt.items())])
    return Case(tag, family, op, n_in, n_out, K, cin, cout, occ, opt)


CASES = [
    # register-gather (spconv_rg.hip): forward image and input-gradient image of the weight, once through out_rows
    _c("rg", "fwd", 1000, 257, 27, 32, 64, image="fwd"), _c("rg", "fwd", 1000, 257, 27, 32, 64, image="dgrad"),
    _c("rg", "fwd", 65, 130, 8, 64, 32, image="fwd"), _c("rg", "fwd", 65, 130, 8, 64, 32, image="dgrad"),
    _c("rg", "fwd", 300, 300, 125, 64, 64, image="fwd"), _c("rg", "fwd", 300, 300, 125, 64, 64, image="dgrad"),
    _c("rg", "fwd", 1000, 257, 27, 32, 64, image="fwd", perm=1),
    # stem (stem.hip): exact-fp32 chains below 32 768 rows, matrix cores from there on
    _c("stem_fp32", "fwd", 1100, 1000, 125, 3, 32, 0.12), _c("stem_fp32", "wgrad", 1100, 1000, 125, 3, 32, 0.12),
    _c("stem_fp32", "fwd", 1100, 1000, 27, 4, 32), _c("stem_fp32", "wgrad", 1100, 1000, 27, 4, 32),
    _c("stem_mfma", "fwd", 30000, STEM_MFMA_ROWS, 125, 3, 32, 0.12), _c("stem_mfma", "wgrad", 30000, STEM_MFMA_ROWS, 125, 3, 32, 0.12),
    _c("stem_mfma", "fwd", 30000, STEM_MFMA_ROWS, 27, 1, 32), _c("stem_mfma", "wgrad", 30000, STEM_MFMA_ROWS, 27, 1, 32),
    # weight-stationary (spconv_ws.hip); the swap launches run on the stride-2 map (n_in, n_out, occ come from the map)
    _c("ws", "fwd", 350, 300, 27, 128, 64, swap=0, direct=0),
    _c("ws", "fwd", 0, 0, 8, 64, 96, swap=1, direct=0, s2="holes"), _c("ws", "fwd", 0, 0, 8, 64, 96, swap=1, direct=1, s2="full"),
    # tile-list (spconv_tl.hip): split launches of the small tables, one persistent multi-tile launch with batch-norm partial sums
    _c("tl", "fwd", 230, 200, 27, 48, 128, split=1), _c("tl", "fwd", 40, 1, 27, 32, 32, split=1), _c("tl", "fwd", 4000, 4100, 27, 32, 512, split=0, bn=1),
    # pair-array weight gradient (wgrad_tl.hip)
    _c("wgrad_tl", "wgrad", 1100, 1000, 27, 64, 20, swap=0), _c("wgrad_tl", "wgrad", 0, 0, 8, 64, 96, swap=1, s2="holes"),
    _c("wgrad_tl", "wgrad", 700, 700, 1, 96, 256, identity=1),
    # first-generation weight gradient (spconv.hip), scalar gather
    _c("wgrad1", "wgrad", 1100, 1000, 27, 6, 32, counts=0), _c("wgrad1", "wgrad", 1100, 1000, 27, 6, 32, counts=1),
    # dense 1x1 (dense.hip): forward image and input-gradient image
    _c("dense", "fwd", 257, 257, 1, 8, 20, identity=1, image="fwd"), _c("dense", "fwd", 257, 257, 1, 8, 20, identity=1, image="dgrad"),
    _c("dense", "fwd", 257, 257, 1, 768, 96, identity=1, image="fwd"), _c("dense", "fwd", 257, 257, 1, 768, 96, identity=1, image="dgrad"),
]


def _both(family, *a, **opt):
    return [_c(family, "fwd", *a, image="fwd", **opt), _c(family, "fwd", *a, image="dgrad", **opt)]


# The instances the shipped networks launch (test_conv_census_cpu.py lists them and fails when one has no case here): per instance
# the smallest shape that reaches it -- a few hundred rows, split tile-list launches (the persistent launch runs the same instance),
# the hand-made 30 % tables, the stride-2 map for the K = 8 launches.  In the comments <..> are the template arguments the channel
# counts select: tile-list <NW, KS> (+ "ragged"), weight-stationary <NW, KS>, pair-array weight gradient <MB, NB>.
CASES += (
    # tile-list, K = 27, both weight images: <3,3> 96->96, <3,4> 128->96, <4,3> 96->128 and 192->128 (two chunks), <4,4> 128->128,
    # 256->256 (two chunks), 384->256 (three)
    _both("tl", 230, 200, 27, 96, 96, split=1) + _both("tl", 230, 200, 27, 128, 96, split=1) + _both("tl", 230, 200, 27, 96, 128, split=1)
    + _both("tl", 230, 200, 27, 192, 128, split=1) + _both("tl", 230, 200, 27, 128, 128, split=1)
    + _both("tl", 230, 200, 27, 256, 256, split=1) + _both("tl", 230, 200, 27, 384, 256, split=1)
    # ... the narrow decoders of 34A / 34B: <2,2> 64->64, <2,3> 96->64, <2,4> 128->64, <3,2> 64->96; 18D's input gradient 384 -> 416
    # is <1,4> (13 column groups of 32), here 128->32; its ragged 416-channel contraction <4,4,ragged>
    + [_c("tl", "fwd", 230, 200, 27, 64, 64, split=1), _c("tl", "fwd", 230, 200, 27, 96, 64, split=1),
       _c("tl", "fwd", 230, 200, 27, 128, 64, split=1), _c("tl", "fwd", 230, 200, 27, 64, 96, split=1),
       _c("tl", "fwd", 230, 200, 27, 128, 32, split=1), _c("tl", "fwd", 230, 200, 27, 416, 128, split=1)]
    # ... K = 8 on the transposed side of the stride-2 map, and the taller tiles: 64 rows (what osn_tile_rows hands out from 86 k
    # rows on; still three workgroups per CU at 96 columns) and 88 rows, the tallest (two)
    + [_c("tl", "fwd", 0, 0, 8, 256, 128, split=1, s2="holes"), _c("tl", "fwd", 0, 0, 8, 128, 96, split=1, s2="full"),
       _c("tl", "fwd", 330, 300, 27, 96, 96, split=1, bm=64), _c("tl", "fwd", 330, 300, 27, 96, 96, split=1, bm=88),
       _c("tl", "fwd", 330, 300, 27, 128, 96, split=1, bm=88)]
    # weight-stationary: <1,1> 32->32, <1,2> 64->32, <1,4> 128->32, <2,2> 64->64, <2,3> 96->64, <3,3> 96->96, <3,4> 128->96,
    # <4,2> 64->128, <4,3> 192->128, <4,4> 256->256; swap and direct launches at K = 8
    + [_c("ws", "fwd", 350, 300, 27, ci, co, swap=0, direct=0) for ci, co in ((32, 32), (64, 32), (128, 32), (64, 64), (96, 64), (96, 96),
                                                                              (128, 96), (64, 128), (192, 128), (256, 256))]
    + [_c("ws", "fwd", 0, 0, 8, 256, 128, swap=1, direct=0, s2="holes"), _c("ws", "fwd", 0, 0, 8, 128, 96, swap=1, direct=1, s2="full"),
       _c("ws", "fwd", 0, 0, 8, 32, 32, swap=1, direct=1, s2="full")]
    # register-gather: the 32->32 instance (the only one with three workgroups per CU)
    + _both("rg", 1000, 257, 27, 32, 32) + [_c("rg", "fwd", 65, 130, 8, 32, 32, image="fwd")]
    # dense 1x1: KS = 2, KS = 3 (two chunks), KS = 4 (three chunks)
    + [_c("dense", "fwd", 257, 257, 1, 64, 128, identity=1, image="fwd"), _c("dense", "fwd", 257, 257, 1, 192, 128, identity=1, image="fwd")]
    + _both("dense", 257, 257, 1, 384, 256, identity=1)
    # pair-array weight gradient: <1,1> <1,2> <2,2> <2,4> <3,2> <3,3> <4,2> <4,3> <4,4>, wider than one workgroup tile from 192 on
    + [_c("wgrad_tl", "wgrad", 350, 300, 27, ci, co, swap=0) for ci, co in ((32, 32), (32, 64), (64, 64), (64, 128), (96, 64), (96, 96),
                                                                           (128, 64), (128, 96), (128, 128), (192, 128), (256, 256), (384, 256))]
    + [_c("wgrad_tl", "wgrad", 0, 0, 8, 256, 128, swap=1, s2="holes"), _c("wgrad_tl", "wgrad", 0, 0, 8, 32, 32, swap=1, s2="full"),
       _c("wgrad_tl", "wgrad", 700, 700, 1, 128, 128, identity=1), _c("wgrad_tl", "wgrad", 700, 700, 1, 32, 64, identity=1)]
    # first-generation weight gradient with 16-byte loads on both operands, 1 - 4 tiles per wave: the heads (32 / 64 / 96 / 128 -> 768)
    # and 18D's 416 -> 384 shortcut, all identity maps
    + [_c("wgrad1", "wgrad", 300, 300, 1, ci, co, identity=1, counts=0) for ci, co in ((32, 768), (64, 768), (96, 768), (416, 384))]
    # first-generation output-stationary kernel (spconv.hip: spconv_fwd_x6_kernel<WM, WN, TN>), which the narrow decoders of 34A / 34B
    # run between 8192 and 65536 rows: <2,2,1> (33 - 64 columns), <2,2,2> (from 4096 rows, 96 columns), <4,1,2> / <4,1,3> (from 32768
    # rows, 64 / 96 columns; thin tables keep the float64 reference small)
    + [_c("x6", "fwd", 350, 300, 27, 128, 64), _c("x6", "fwd", 4300, 4100, 27, 64, 96, 0.05),
       _c("x6", "fwd", 30000, 32800, 27, 128, 64, 0.03), _c("x6", "fwd", 30000, 32800, 27, 64, 96, 0.03)]
    # stem from 4096 rows on: four lanes per output row (stem_fwd4_kernel)
    + [_c("stem_fp32", "fwd", 4300, 4100, 125, 3, 32, 0.12), _c("stem_fp32", "fwd", 4300, 4100, 27, 4, 32)]
)
CASE_IDS = [c.id for c in CASES]


def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7FFFFFFF


@functools.lru_cache(maxsize=None)
def stride2_map(variant):
    """-> (strided table int32 [8, n_coarse] whose entries are fine rows, n_fine): the 2^3 stride-2 map of ~600 voxels from the
    oracle's coordinate manager, plus a tenth more coarse rows without any child (input rows nothing references, on the transposed
    side); "holes": a tenth of the pairs removed as well, so that some fine rows have no pair."""
    v = syn.shuffled(syn.grid_voxels(syn.room_points(11, n_pts=700), 0.1), 11)
    cm = oc.CoordinateManager(syn.batch_coords([v]))
    t = cm.kmap(1, 2, 2)
    n_fine = cm.level(1).shape[0]
    rng = np.random.default_rng(5)
    extra = max(8, t.shape[1] // 10)
    t = np.concatenate([t, np.full((8, extra), -1, np.int32)], 1)
    t = t[:, rng.permutation(t.shape[1])]
    if variant == "holes":
        t = np.where((rng.random(t.shape) < 0.1) & (t >= 0), -1, t).astype(np.int32)
    t = np.ascontiguousarray(t)
    return t, n_fine


@functools.lru_cache(maxsize=None)
def case_table(shape_key):
    """int32 [K, n_out] numpy table (shared, never modified) of a case's shape, nbr[k, o] = input row or -1; None for the identity map.
    Hand-made: random entries at the case's occupancy, drawn from nine tenths of the input rows (the others are referenced by
    nothing), output row 2 without any neighbour."""
    n_in, n_out, K, occ, s2, identity = shape_key
    if identity:
        return None
    if s2:
        t, n_fine = stride2_map(s2)
        nbr = oc.transpose_table(t, n_fine)                 # the transposed convolution's table: coarse -> fine
    else:
        g = torch.Generator().manual_seed(_seed("table", shape_key))
        pool = torch.randperm(n_in, generator=g)[:max(1, (n_in * 9) // 10)]
        nbr = pool[torch.randint(0, pool.shape[0], (K, n_out), generator=g)].int()
        nbr[torch.rand(K, n_out, generator=g) >= occ] = -1
        if n_out > 3:
            nbr[:, 2] = -1
        nbr = nbr.numpy()
    return nbr


def resolve(case):
    """The case with the row counts of its map filled in, and its table."""
    s2 = case.opt.get("s2")
    if s2:
        t, n_fine = stride2_map(s2)
        case = case._replace(n_in=t.shape[1], n_out=n_fine)
    nbr = case_table((case.n_in, case.n_out, case.K, case.occ, s2, bool(case.opt.get("identity"))))
    return case, nbr


@functools.lru_cache(maxsize=5)
def _operands(n_in, n_out, K, cin, cout, occ, kind):
    g = torch.Generator().manual_seed(_seed("operands", n_in, n_out, K, cin, cout, kind))
    feats = adversarial(kind, n_in, cin, g)
    w = adversarial_weight(kind, K, cin, cout, g, K * cin * occ)
    gout = adversarial(kind if kind != "cancellation" else "row_scales", n_out, cout, g)
    return feats, w, gout


def operands(case, kind):
    """(features [n_in, cin], weight [K, cin, cout], output gradient [n_out, cout]) of a resolved case; shared, never modified."""
    return _operands(case.n_in, case.n_out, case.K, case.cin, case.cout, case.occ if case.K > 1 else 1.0, kind)


@functools.lru_cache(maxsize=5)
def _reference(n_in, n_out, K, cin, cout, occ, s2, identity, kind):
    nbr = case_table((n_in, n_out, K, occ, s2, identity))
    feats, w, gout = _operands(n_in, n_out, K, cin, cout, occ if K > 1 else 1.0, kind)
    return abs_sum_bounds(nbr, feats, w, gout, with_gin=False)


def reference(case, kind):
    """abs_sum_bounds of a resolved case's operands, computed once per (shape, kind): the forward and the weight-gradient case of one
    shape share it."""
    return _reference(case.n_in, case.n_out, case.K, case.cin, case.cout, case.occ, case.opt.get("s2"), bool(case.opt.get("identity")), kind)


# -------------------------------------------------------------------------------------------------------------- the launches
class Launch:
    """The kernel of a resolved case, ready to run on features (and an output gradient) that live on `device`: the GPU in
    test_gpu_conv_bounds.py, the host under the null runtime of the instance census (conv_census.py)."""

    def __init__(self, case, nbr, device):
        from openscene_amd import ops
        self.ops, self.case, self.nbr_np = ops, case, nbr
        d = device
        self.nbr = torch.from_numpy(np.ascontiguousarray(nbr)).to(d) if nbr is not None else None
        self.tl = self.rows = self.counts = None
        f, o = case.family, case.opt
        if f == "rg" and o.get("perm"):
            g = torch.Generator().manual_seed(3)
            perm = torch.randperm(case.n_out, generator=g)
            self.nbr, self.rows = self.nbr[:, perm.to(d)].contiguous(), perm.int().to(d)
        if f == "tl" or (f in ("ws", "wgrad_tl") and not o.get("swap") and not o.get("identity")):
            self.tl = ops.tile_lists(self.nbr, bm=o.get("bm"))   # (bm: a tile height other than osn_tile_rows' for this row count)
        if o.get("s2") and f != "tl":                        # the lists of the strided convolution this launch mirrors
            self.tl = ops.tile_lists(torch.from_numpy(stride2_map(o["s2"])[0]).to(d))
        if f == "wgrad1" and o.get("counts"):
            self.counts = ops.kmap_count(self.nbr)
        if f == "tl":                                        # the case is where its name says: a split launch, or one persistent launch
            wsb = int(ops._cached("osn_spconv_fwd_tl_ws_bytes", case.n_out, case.K, case.cout, self.tl.bm))
            assert (wsb > 512) == bool(o["split"]) and (o["split"] or self.tl.n_tiles > 1)
        if f == "rg":
            assert ops.rg_eligible(case.K, case.cin, case.cout, case.n_in)
        if f in ("stem_fp32", "stem_mfma"):
            assert ops.stem_eligible(case.K, case.cin, case.cout) and (case.n_out >= 32768) == (f == "stem_mfma")

    def image(self, w):
        """The weight image the launch multiplies with: the forward image of w, or the input-gradient image of the transposed weight
        (the same matrix per offset, through the other preparation path)."""
        ops = self.ops
        if self.case.opt.get("image") == "dgrad":
            return ops.weight_prep_tl(w.transpose(1, 2).contiguous(), flip=False, want_fwd=False)[1]
        return ops.weight_prep_tl(w, want_dgrad=False)[0]

    def fwd(self, feats, w, bn_partial=None):
        ops, c, o = self.ops, self.case, self.case.opt
        if c.family in ("stem_fp32", "stem_mfma"):
            return ops.stem_conv_fwd(feats, w, self.nbr, c.n_out)
        if c.family == "x6":
            assert ops.x6_eligible(c.K, c.cin, c.cout, c.n_out)
            return ops.spconv_fwd_x6(feats, ops.weight_prep_x6(w), self.nbr, c.n_out)
        wp = self.image(w)
        if c.family == "rg":
            return ops.spconv_fwd_rg(feats, wp, self.nbr, c.n_out, c.cout, out_rows=self.rows)
        if c.family == "ws":
            return ops.spconv_fwd_ws(feats, wp, self.tl, None if o["direct"] else self.nbr, c.n_out, c.K, c.cout,
                                     swap=bool(o["swap"]), direct=bool(o["direct"]))
        if c.family == "tl":
            return ops.spconv_fwd_tl(feats, wp, self.tl, c.n_out, c.K, c.cout, bn_partial=bn_partial)
        assert c.family == "dense" and ops.dense_eligible(c.cin, c.cout)
        return ops.dense_fwd(feats, wp, c.cout)

    def wgrad(self, feats, gout):
        ops, c, o = self.ops, self.case, self.case.opt
        if c.family in ("stem_fp32", "stem_mfma"):
            return ops.stem_conv_wgrad(feats, gout, self.nbr, c.K)
        if c.family == "wgrad_tl":
            return ops.spconv_wgrad_tl(feats, gout, self.tl, c.K, swap=bool(o.get("swap")))
        assert c.family == "wgrad1"
        return ops.spconv_wgrad(feats, gout, self.nbr, c.K, self.counts)


# ------------------------------------------------------------------------------------------- the batched weight-gradient reduction
# What every executor backward runs: osn_spconv_wgrad_tl_partial per convolution, then osn_wgrad_tl_reduce_batch over all of them, one
# launch per 32 jobs.  BATCH_JOBS live jobs reach the second launch with a ragged last batch (one job); one of them is a map without
# any pair, and one more entry has no rows at all (its job is skipped: gW is zeroed by the first call).
BATCH_JOBS = 33
EMPTY_MAP = _c("wgrad_tl", "wgrad", 120, 100, 27, 64, 64, 0.0, swap=0)        # rows on both sides, every table entry -1
NO_ROWS = _c("wgrad_tl", "wgrad", 0, 0, 1, 64, 32, identity=1)


def batch_plan():
    """[(case, operand kind)]: the pair-array weight-gradient cases in turn (mixed shapes, swap launches, identity maps) with the
    operand kinds in turn, the map without pairs as the last live job, then the entry without rows."""
    wg = [c for c in CASES if c.family == "wgrad_tl"]
    plan = [(wg[i % len(wg)], KINDS[i % len(KINDS)]) for i in range(BATCH_JOBS - 1)]
    return plan + [(EMPTY_MAP, "row_scales"), (NO_ROWS, "row_scales")]


def batch_operands(case, kind):
    """(features, output gradient) of a resolved case of batch_plan()."""
    if case.id in (EMPTY_MAP.id, NO_ROWS.id):
        g = torch.Generator().manual_seed(_seed("batch", case.id))
        return adversarial(kind, case.n_in, case.cin, g), adversarial(kind, case.n_out, case.cout, g)
    feats, _w, gout = operands(case, kind)
    return feats, gout


def batch_entries(launch_of, place, zeros=False):
    """[(Launch, features, output gradient)] of batch_plan(), the input of batched_wgrad.  launch_of(case) -> (resolved case, table,
    Launch); place(tensor) -> the operand where the launch wants it; zeros: operands of the right shapes only (the instance census)."""
    entries = []
    for case, kind in batch_plan():
        rc, _nbr, run = launch_of(case)
        if zeros:
            feats, gout = torch.zeros(rc.n_in, rc.cin), torch.zeros(rc.n_out, rc.cout)
        else:
            feats, gout = batch_operands(rc, kind)
        entries.append((run, place(feats), place(gout)))
    return entries


class WgradJob(ctypes.Structure):                # osn_wgrad_job (include/openscene_amd.h)
    _fields_ = [("partial", ctypes.c_void_p), ("range", ctypes.c_void_p), ("gW", ctypes.c_void_p), ("K", ctypes.c_int32),
                ("cin", ctypes.c_int32), ("cout", ctypes.c_int32), ("ident_items", ctypes.c_int32)]


def batched_wgrad(entries, device):
    """entries: [(Launch of a pair-array weight-gradient case, features, output gradient)] on `device` -> ([gW], the job array):
    one osn_spconv_wgrad_tl_partial per entry, each into a partial buffer of its own, then ONE osn_wgrad_tl_reduce_batch."""
    from openscene_amd import ops
    assert ctypes.sizeof(WgradJob) == 40
    lib = ops._prep(device)
    jobs = (WgradJob * len(entries))()
    partials, out = [], []
    with ops._Dev(device):
        for i, (run, feats, gout) in enumerate(entries):
            c = run.case
            pl = ops.pair_lists(run.tl) if run.tl is not None else None
            gw = torch.full((c.K, c.cin, c.cout), float("nan"), dtype=torch.float32, device=device)
            nbytes = int(ops._cached("osn_spconv_wgrad_tl_ws_bytes", c.K, c.cin, c.cout))
            partial = torch.empty(nbytes, dtype=torch.uint8, device=device)
            ops.check(lib.osn_spconv_wgrad_tl_partial(ops._p(feats), ops._p(gout), ops._p(pl), int(bool(c.opt.get("swap"))), ops._p(gw),
                                                      feats.shape[0], gout.shape[0], c.K, c.cin, c.cout, ops._p(partial), nbytes,
                                                      ctypes.addressof(jobs) + i * ctypes.sizeof(WgradJob), ops._stream(device)),
                      "osn_spconv_wgrad_tl_partial")
            partials.append(partial)
            out.append(gw)
        ops.check(lib.osn_wgrad_tl_reduce_batch(ctypes.addressof(jobs), len(entries), ops._stream(device)), "osn_wgrad_tl_reduce_batch")
    return out, jobs
