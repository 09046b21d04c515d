"""Autograd glue: each Function's forward/backward is one or two C-ABI calls on
the current HIP stream (backward runs on autograd's thread; the library is
stateless so that is safe)."""
import os
import threading

import torch
from torch.autograd import Function

from . import ops, precision

# Kernels / arithmetic of the forward and input-gradient convolutions:
#   "tl"     (default) second-generation kernels: forward / input gradient from per-tile compacted pair lists
#            (weights in registers, output tile in LDS, spconv_tl.hip) on the large maps, weight gradient from
#            per-offset pair arrays on the bf16 MFMA (wgrad_tl.hip) on every map; the other families (1x1, weight-stationary,
#            register-gather, stem) and the order they are tried in: conv_kernels below
#   "bf16x6" output-stationary kernel over the dense neighbour table, three-way bf16 split of both operands,
#            six bf16 MFMAs per product block, fp32 accumulate: fp32-level accuracy
#   "fp32"   the same kernel on v_mfma_f32_32x32x2_f32 (exact fp32 products, 157 TF peak)
CONV_MODE = os.environ.get("OSN_CONV_MODE", "tl")
# Tile-list kernel, forward / input gradient: on the tables of at least this many rows (measured: 20-30 % faster on the 100 k-row
# maps, a tie at 48 k rows, slower below) ...
TL_FWD_MIN_ROWS = 65536
# ... and from this many rows on when both channel counts are at least 96 (measured with the per-width channel chunks of
# round 3, profiles/r03_s8: 48 k rows 96 -> 96 121 us against 134 us, 128 -> 96 143 / 164; 12.9 k rows 128 -> 128 63 / 78,
# 192 -> 128 88 / 104; narrower layers -- 64 -> 64: 39 / 34, 32 -> 32: 67 / 34 -- stay on the output-stationary kernel)
TL_MID_MIN_ROWS = 8192


# Weight-stationary kernel (spconv_ws.hip) for the launches that write at most this many rows (measured, profiles/r03_s9:
# 3 k rows 128 -> 128 34 us against 45, 256 -> 256 69 / 106-122; 700 rows 256 -> 256 30 / 43; a tie at 12.9 k rows; the limit
# 8192 against 4096 / 16384: L235k-34C step 25.5 / 26.2 / 25.6 ms, 8-scene batch 49.5 / 49.8 / 49.7, S100k 9.90 / 9.89 / 10.01), and --
# without a row limit -- for the launches that write the fine side of a 2^3 stride-2 map, where every row has exactly one
# pair and the result rows go straight to the output (100 k rows 96 -> 96: 32 us against 70; 48 k rows 128 -> 96: 20 / 62)
WS_MAX_ROWS = 8192


def ws_kernel(K, c_src, c_dst, n_src, n_dst, fine_unique, dst_fine):
    """"ws_direct" / "ws" / None: the weight-stationary kernel for a launch that gathers n_src rows of c_src channels and
    writes n_dst rows of c_dst channels (same rule as csrc/net.hip:ws_kernel; the shape predicate under both is one C export)."""
    if K <= 1 or not ops.tl_eligible(K, c_src, c_dst, n_src):
        return None
    if fine_unique and dst_fine:
        return "ws_direct"
    if 0 < n_dst <= WS_MAX_ROWS:
        return "ws"
    return None


def tl_rows_ok(n_rows, c_a, c_b):
    """Is a table of n_rows rows big enough for the tile-list kernel on a conv between c_a and c_b channels?"""
    return n_rows >= TL_FWD_MIN_ROWS or (n_rows >= TL_MID_MIN_ROWS and min(c_a, c_b) >= 96)
# Backward of a convolution on a map of at most this many rows: the weight gradient (plan + kernel + reduce) runs on an
# auxiliary stream beside the input gradient (+ its reduce); the node forks after `gout` is ready and joins before it
# returns, so nothing outside sees the second stream.  OFF by default (0): measured on S100k (tools/ab_wall.sh, 2 rounds)
# 14.78 / 14.18 ms with 40000 against 14.31 / 14.29 ms without -- the deep levels are bound by the host's launch rate,
# not by the GPU, so there is nothing to overlap; 70000 and 200000 are slower (15.0 ms).  Results are bitwise identical.
WGRAD_OVERLAP_MAX_ROWS = 0


# kernel name -> layout of the weight image it multiplies with (the other kernels read the fp32 weight)
_IMAGE = {"dense": ops.PREP_TL, "ws_direct": ops.PREP_TL, "tl": ops.PREP_TL, "rg": ops.PREP_TL, "ws": ops.PREP_TL, "x6": ops.PREP_X6}


_plans = {}


def conv_kernels(K, cin, cout, n_in, n_out, transposed, fine_unique, need_dgrad=True, have_lists_fwd=True, have_lists_bwd=True,
                 have_pairs=True):
    """_plan_kernels, remembered per argument set and per state of everything it reads: the thresholds and rules above, which
    tests and tools set, and the shape predicates of ops, which host-logic tests swap (the per-module path is host-bound, and a
    step asks the same ~40 questions again)."""
    key = (K, cin, cout, n_in, n_out, transposed, fine_unique, need_dgrad, have_lists_fwd, have_lists_bwd, have_pairs,
           CONV_MODE, TL_FWD_MIN_ROWS, TL_MID_MIN_ROWS, WS_MAX_ROWS, ws_kernel, tl_rows_ok,
           ops.stem_eligible, ops.dense_eligible, ops.tl_eligible, ops.rg_eligible, ops.x6_eligible)
    plan = _plans.get(key)
    if plan is None:
        plan = _plans[key] = _plan_kernels(*key[:11])
    return plan


def _plan_kernels(K, cin, cout, n_in, n_out, transposed, fine_unique, need_dgrad, have_lists_fwd, have_lists_bwd, have_pairs):
    """(forward, input-gradient, weight-gradient) kernel of a convolution, by the names Executor.kernels() reports; "generic": the
    table kernel ops.spconv_fwd, which the executor does not have; "none": no input gradient wanted.  have_*: what the map handed in
    (tile lists per direction, pair arrays).  THE rule of the per-module path; csrc/net.hip:pick_kernel / pick_wgrad are its twins,
    tests/test_executor.py::test_both_paths_plan_the_same_kernels holds the two together.  The shape predicates are no twins: both
    paths ask the library's osn_*_ok exports (ops.*_eligible here)."""
    tl_mode = CONV_MODE == "tl"
    lists_mode = tl_mode and K > 1 and ops.tl_eligible(K, cin, cout, n_in)

    def pick(c_src, c_dst, n_src, n_dst, dst_fine, have_lists):
        """The kernel of a launch that gathers n_src rows of c_src channels and writes n_dst rows of c_dst channels."""
        if tl_mode and K == 1 and ops.dense_eligible(cin, cout) and ops.dense_eligible(c_src, c_dst):
            return "dense"                          # 1x1 convs (head, shortcuts): the row-wise matrix-product kernel
        if lists_mode:
            both = ops.tl_eligible(K, c_src, c_dst, n_src)
            ws = ws_kernel(K, c_src, c_dst, n_src, n_dst, fine_unique, dst_fine) if have_pairs else None
            if ws == "ws_direct":
                return ws
            # (a layer with 32 channels on one side goes to the register-gather kernel on ANY map size, measured in csrc/net.hip)
            rg = ops.rg_eligible(K, c_src, c_dst, n_src)
            if both and have_lists and tl_rows_ok(n_dst, cin, cout) and not (rg and min(cin, cout) == 32):
                return "tl"
            if rg:
                return "rg"
            if ws:
                return ws
        if CONV_MODE in ("tl", "bf16x6") and ops.x6_eligible(K, c_src, c_dst, n_dst):
            return "x6"
        return "generic"

    if CONV_MODE != "fp32" and ops.stem_eligible(K, cin, cout):
        fwd, wgrad = "stem", "wgrad_stem"
    else:
        fwd = pick(cin, cout, n_in, n_out, transposed, have_lists_fwd)
        # pair-array kernel on every 3^3 / 2^3 map and, on the identity map, for the 1x1 shortcut convs (the 96 -> 768 head stays on
        # the table kernel: 188 us against 215 us measured)
        pairs = have_pairs if K > 1 else cin <= 256 and cout <= 256
        wgrad = "wgrad_tl" if tl_mode and pairs and ops.tl_eligible(K, cin, cout, n_in) else "wgrad"
    return fwd, pick(cout, cin, n_out, n_in, not transposed, have_lists_bwd) if need_dgrad else "none", wgrad


def _launch(name, x, w, n_dst, c_dst, K, nbr, tiles, lists, pairs, swap, pieces=3):
    """Convolution kernel `name` on x -> [n_dst, c_dst] (the Python twin of run_conv in csrc/net.hip).  w: the weight image _IMAGE
    names, else the fp32 weight; nbr / tiles / lists: the destination side's table, tile-ordered table and tile lists; pairs, swap:
    the map's pair arrays and whether this launch walks them the other way; pieces: operand pieces of the four split-bf16 families
    (openscene_amd.precision.pass_pieces: the inference mode of an evaluation-mode pass that records no graph, else the training mode)."""
    tbl, rows, gm = (tiles[1], tiles[0], tiles[2]) if tiles is not None else (nbr, None, None)
    kw = {} if pieces == 3 else {"pieces": pieces}          # (the default mode calls the wrappers as it always did)
    if name == "stem":
        return ops.stem_conv_fwd(x, w, nbr, n_dst)
    if name == "dense":
        return ops.dense_fwd(x, w, c_dst, **kw)
    if name in ("ws", "ws_direct"):
        return ops.spconv_fwd_ws(x, w, pairs, nbr, n_dst, K, c_dst, swap=swap, direct=name == "ws_direct", **kw)
    if name == "tl":
        return ops.spconv_fwd_tl(x, w, lists, n_dst, K, c_dst, **kw)
    if name == "rg":
        return ops.spconv_fwd_rg(x, w, tbl, n_dst, c_dst, out_rows=rows, **kw)
    if name == "x6":
        return ops.spconv_fwd_x6(x, w, tbl, n_dst, out_rows=rows, gmask=gm)
    return ops.spconv_fwd(x, w, tbl, n_dst, out_rows=rows, gmask=gm)


class SparseConvFunction(Function):
    """out[o] = sum_k feats[nbr_fwd[k, o]] @ kernel[k]  ([ME] MinkowskiConvolutionFunction /
    MinkowskiConvolutionTransposeFunction).  kernel: [K, cin, cout], or [cin, cout] when K == 1."""

    @staticmethod
    def forward(ctx, feats, kernel, nbr_fwd, nbr_bwd, flip, n_out, tiles_fwd=None, tiles_bwd=None, counts=None,
                lists_fwd=None, lists_bwd=None, transposed=False, fine_unique=False, pieces=3):
        ctx.save_for_backward(feats, kernel)
        n_in, flip = feats.shape[0], bool(flip)
        K = 1 if kernel.dim() == 2 else kernel.shape[0]
        cin, cout = kernel.shape[-2], kernel.shape[-1]
        # pair arrays of the map: those of the strided / self direction (a transposed conv runs on the arrays of the strided conv it
        # mirrors = its own input-gradient lists, and walks them the other way)
        pairs = lists_bwd if transposed else lists_fwd
        fwd, dgrad, wgrad = conv_kernels(K, cin, cout, n_in, n_out, transposed, fine_unique, ctx.needs_input_grad[0],
                                         lists_fwd is not None, lists_bwd is not None, pairs is not None)

        def image(name, for_dgrad):
            # (for_dgrad: transposed, and on a self map the offsets mirrored -- a 1x1 kernel has one offset)
            return ops.weight_image(kernel, flip and for_dgrad and name != "dense", for_dgrad, _IMAGE[name]) if name in _IMAGE else None
        # Weight images: parameters are served from ops' per-device cache (one launch per optimizer step for the whole model), so
        # the input-gradient image is requested here too and is part of that launch.  The cache prepares a model's images in the
        # order of their first request, and that order stays what it was: the input-gradient image first, but behind the forward
        # image when it is a tile-list image after a tile-list / weight-stationary forward, or a first-generation image.  The
        # latter after any other forward kernel (the stem with an input gradient, odd shapes: no layer of the U-Nets) is asked for
        # in the backward pass.
        late = dgrad == "x6" or (dgrad == "tl" and fwd in ("tl", "ws", "ws_direct"))
        wd = None if late else image(dgrad, True)
        wf = image(fwd, False)
        if late and (dgrad == "tl" or fwd == "x6"):
            wd = image(dgrad, True)
        # the cached images are shared and refreshed in place: remember which version of the kernel the image kept for the backward
        # pass belongs to (a weight changed through .data between forward and backward bypasses autograd's own saved-tensor check)
        ctx.kver = (kernel._version, kernel.data_ptr())
        # the input gradient is a convolution of the output gradient over the map's other side; on a self map (flip) it keeps the
        # direction of the pair arrays and takes the mirrored weight image
        ctx.dgrad = (dgrad, wd, nbr_bwd, tiles_bwd, lists_bwd, pairs, transposed if flip else not transposed)
        ctx.wgrad = (wgrad, nbr_fwd, counts, transposed, flip)
        ctx.pieces = pieces                    # the backward pass runs in the forward's mode, wherever backward() is called
        return _launch(fwd, feats, wf if wf is not None else kernel, n_out, cout, K, nbr_fwd, tiles_fwd, lists_fwd, pairs, transposed, pieces)

    @staticmethod
    def backward(ctx, gout):
        feats, kernel = ctx.saved_tensors
        dgrad, wd, nbr_bwd, tiles_bwd, lists_bwd, pairs, swap_b = ctx.dgrad
        wgrad, nbr_fwd, counts, swap, flip = ctx.wgrad
        gout = gout.contiguous()
        gin = gk = None
        pieces = ctx.pieces
        kw = {} if pieces == 3 else {"pieces": pieces}          # (the default mode calls the wrappers as it always did)
        K = 1 if kernel.dim() == 2 else kernel.shape[0]
        n_in, cin = feats.shape
        if wd is not None and ctx.kver != (kernel._version, kernel.data_ptr()):
            raise RuntimeError("a convolution kernel changed between its forward and its backward pass (version %d -> %d): "
                               "the input-gradient weight image kept from the forward is stale" % (ctx.kver[0], kernel._version))

        def weight_grad():
            if wgrad == "wgrad_stem":
                gw = ops.stem_conv_wgrad(feats, gout, nbr_fwd, K)
            elif wgrad == "wgrad_tl":
                gw = ops.spconv_wgrad_tl(feats, gout, pairs, K, swap=swap, **kw) if K > 1 else ops.spconv_wgrad_tl(feats, gout, None, 1, **kw)
            else:
                gw = ops.spconv_wgrad(feats, gout, nbr_fwd, K, counts)
            return gw.reshape(kernel.shape)

        side = None
        if ctx.needs_input_grad[1]:
            if (ctx.needs_input_grad[0] and gout.is_cuda
                    and max(n_in, gout.shape[0]) <= WGRAD_OVERLAP_MAX_ROWS):
                main = torch.cuda.current_stream(gout.device)
                side = ops.side_stream(gout.device)
                side.wait_stream(main)                    # fork: gout (and everything before it) is ready
                with ops.on_stream(side):
                    gk = weight_grad()
            else:
                gk = weight_grad()
        if ctx.needs_input_grad[0]:
            if wd is None:
                wd = ops.weight_image(kernel, flip, True, ops.PREP_X6) if dgrad == "x6" else ops.weight_transpose(kernel, flip)
            gin = _launch(dgrad, gout, wd, n_in, cin, K, nbr_bwd, tiles_bwd, lists_bwd, pairs, swap_b, pieces)
        if side is not None:
            main.wait_stream(side)                        # join: later work on this stream sees the weight gradient
        return gin, gk, None, None, None, None, None, None, None, None, None, None, None, None


class BatchNormActFunction(Function):
    """y = act(BN(x) [+ residual]) in one pass over x; batch statistics in training
    (running buffers updated in place like torch.nn.BatchNorm1d), running statistics in eval."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, residual, training, momentum, eps, relu):
        x = x.contiguous()
        if training:
            y, mean, var = ops.bn_forward_train(x, gamma, beta, eps, residual, relu, running_mean, running_var, momentum)
        else:
            mean, var = running_mean, running_var
            y = ops.bn_apply(x, mean, var, gamma, beta, eps, residual, relu)
        # bn -> relu without a residual: the backward pass recomputes the mask (y > 0) from x instead of reading y
        ctx.save_for_backward(x, y if (relu and residual is not None) else None, mean, var, gamma, beta if relu else None)
        ctx.cfg = (bool(training), float(eps), bool(relu), residual is not None)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, y, mean, var, gamma, beta = ctx.saved_tensors
        training, eps, relu, has_res = ctx.cfg
        want_gres = has_res and ctx.needs_input_grad[5]
        gx, gres, ggamma, gbeta = ops.bn_backward(x, y, gy.contiguous(), mean, var, gamma, eps, relu, training,
                                                  want_gres, beta=beta if (relu and not has_res) else None)
        return gx, ggamma, gbeta, None, None, gres, None, None, None, None


class ReluFunction(Function):
    """Stand-alone ME.MinkowskiReLU (models/mink_unet.py:114) of the un-fused module chain."""

    @staticmethod
    def forward(ctx, x):
        y = ops.relu_fwd(x)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, gy):
        (y,) = ctx.saved_tensors
        return ops.relu_bwd(y, gy)


class AddFunction(Function):
    """Row-aligned a + b of two feature matrices on one coordinate map (the un-fused residual `out += residual`)."""

    @staticmethod
    def forward(ctx, a, b):
        return ops.add(a, b)

    @staticmethod
    def backward(ctx, g):
        return g, g


class Cat2Function(Function):
    """ME.cat of two tensors (models/mink_unet.py:147,155,163,171): one launch forward, one launch backward."""

    @staticmethod
    def forward(ctx, a, b):
        ctx.widths = (a.shape[1], b.shape[1])
        return ops.cat2(a, b)

    @staticmethod
    def backward(ctx, g):
        ca, cb = ctx.widths
        if not ctx.needs_input_grad[0] or not ctx.needs_input_grad[1]:
            g = g.contiguous()
            return (g[:, :ca].contiguous() if ctx.needs_input_grad[0] else None,
                    g[:, ca:].contiguous() if ctx.needs_input_grad[1] else None)
        return ops.cat2_bwd(g, ca, cb)


class LocalPoolFunction(Function):
    """[ME] MinkowskiSumPooling / AvgPooling / MaxPooling over a kernel map: one launch forward, one backward (a gather through
    the inverse table in ascending forward offset: no atomics).  `cnt` (avg) and `arg` (max) are kept for the backward pass."""

    @staticmethod
    def forward(ctx, x, nbr_fwd, nbr_bwd, flip, mode, cnt):
        y, arg = ops.pool_fwd(x, nbr_fwd, mode)
        ctx.cfg = (nbr_bwd, bool(flip), mode, cnt)
        ctx.save_for_backward(arg)
        return y

    @staticmethod
    def backward(ctx, gy):
        nbr_bwd, flip, mode, cnt = ctx.cfg
        (arg,) = ctx.saved_tensors
        return ops.pool_bwd(gy, nbr_bwd, flip, mode, cnt=cnt, arg=arg), None, None, None, None, None


class GlobalPoolFunction(Function):
    """[ME] MinkowskiGlobalSumPooling / AvgPooling / MaxPooling: one row per batch of a CoordinateManager.batch_index."""

    @staticmethod
    def forward(ctx, x, index, mode):
        y, arg = ops.gpool_fwd(x, index.order, index.offsets, mode)
        ctx.cfg = (index, mode, x.shape[0])
        ctx.save_for_backward(arg)
        return y

    @staticmethod
    def backward(ctx, gy):
        index, mode, n = ctx.cfg
        (arg,) = ctx.saved_tensors
        return ops.gpool_bwd(gy, index.rank, index.offsets, n, mode, arg=arg), None, None


class BroadcastFunction(Function):
    """[ME] MinkowskiBroadcastAddition / Multiplication: y[i] = x[i] (+ | *) pooled[batch(i)]."""

    @staticmethod
    def forward(ctx, x, pooled, index, op):
        ctx.cfg = (index, op)
        ctx.save_for_backward(x if op == "mul" else None, pooled if op == "mul" else None)
        return ops.broadcast_fwd(x, pooled, index.rank, op)

    @staticmethod
    def backward(ctx, gy):
        index, op = ctx.cfg
        x, pooled = ctx.saved_tensors
        gx = gg = None
        if ctx.needs_input_grad[0]:
            gx = gy if op == "add" else ops.broadcast_fwd(gy, pooled, index.rank, "mul")
        if ctx.needs_input_grad[1]:
            gg = ops.broadcast_bwd_pooled(gy, x, index.order, index.offsets)
        return gx, gg, None, None


def local_pool(x, maps, mode, cnt=None):
    """maps = CoordinateManager.kmap(...); mode "sum" / "avg" / "max"; cnt = .pool_counts(...) for "avg"."""
    nbr_fwd, nbr_bwd, flip = maps
    if nbr_fwd is None:
        raise ValueError("local pooling needs a kernel map (kernel_size 1 pools nothing)")
    return LocalPoolFunction.apply(x, nbr_fwd, nbr_bwd, flip, mode, cnt)


def global_pool(x, index, mode):
    """index = CoordinateManager.batch_index(stride) of x's rows."""
    return GlobalPoolFunction.apply(x, index, mode)


def broadcast(x, pooled, index, op):
    """op "add" / "mul"; pooled [B, C] on the batches of index."""
    if pooled.dim() != 2 or pooled.shape[0] != index.ids.shape[0] or pooled.shape[1] != x.shape[1]:
        raise ValueError("broadcast: pooled features %s do not match %d batches of %d columns"
                         % (tuple(pooled.shape), index.ids.shape[0], x.shape[1]))
    return BroadcastFunction.apply(x, pooled, index, op)


# ---- points in and out of the grid (field.py).  `index` is a field.FieldIndex: rank int32 [N] the voxel row
# of every point, order / offsets the points of every voxel in ascending point index (CSR), first int64 [U] each voxel's first point
class QuantizeFunction(Function):
    """[ME] TensorField.sparse(), SparseTensor(quantization_mode=): the sum or the average of the points of every voxel in ascending
    point index; the backward pass is the gather osn_gpool_bwd performs, with a voxel in the place of a batch."""

    @staticmethod
    def forward(ctx, x, index, mode):
        ctx.cfg = (index, mode)
        return ops.segment_reduce(x, index.order, index.offsets, mode)

    @staticmethod
    def backward(ctx, gy):
        index, mode = ctx.cfg
        return ops.segment_expand(gy, index.rank, index.offsets, mode), None, None


class SubsampleFunction(Function):
    """RANDOM_SUBSAMPLE: the first point's row of every voxel (row indexing, what SparseTensor always did); the gradient goes to
    that point, +0 to the others."""

    @staticmethod
    def forward(ctx, x, first):
        ctx.cfg = (first, x.shape[0])
        return x[first]

    @staticmethod
    def backward(ctx, gy):
        first, n = ctx.cfg
        return gy.new_zeros((n,) + tuple(gy.shape[1:])).index_copy_(0, first, gy), None


class SliceFunction(Function):
    """[ME] SparseTensor.slice: F[i] = x[rank[i]]; the backward pass is the quantisation's ordered sum."""

    @staticmethod
    def forward(ctx, x, index):
        ctx.index = index
        return ops.segment_expand(x, index.rank)

    @staticmethod
    def backward(ctx, gy):
        index = ctx.index
        return ops.segment_reduce(gy, index.order, index.offsets, "sum"), None


class InterpolateFunction(Function):
    """[ME] MinkowskiInterpolation: trilinear interpolation over a field.InterpolationMap; the backward pass walks the map's plan
    (built on the first backward pass, kept on the map).  No gradient with respect to the positions."""

    @staticmethod
    def forward(ctx, x, imap):
        ctx.imap = imap
        return ops.interp_fwd(x, imap.nbr, imap.w)

    @staticmethod
    def backward(ctx, gy):
        imap = ctx.imap
        return ops.interp_bwd(gy, imap.plan(), imap.w, imap.n_in), None


def quantize(x, index, mode):
    """mode "sum" / "avg" / "first" over a field.FieldIndex."""
    if mode == "first":
        return SubsampleFunction.apply(x, index.first)
    return QuantizeFunction.apply(x, index, mode)


def slice_rows(x, index):
    return SliceFunction.apply(x, index)


def interpolate(x, imap):
    if x.dim() != 2 or x.shape[0] != imap.n_in:
        raise ValueError("interpolate: features %s against a map over %d voxel rows" % (tuple(x.shape), imap.n_in))
    return InterpolateFunction.apply(x, imap)


def _hip_eligible(*ts):
    """The elementwise HIP kernels take contiguous float32 device matrices on 16-byte boundaries.  Anything else ON A DEVICE
    (another dtype, a strided view, an odd storage offset) goes to the torch operator of the same name -- MinkowskiEngine
    accepts those too; host tensors are refused by the ops like everywhere else (no CPU fallback)."""
    for t in ts:
        if not t.is_cuda:
            return True                 # -> ops.* raises its usual error
        if t.dtype != torch.float32 or not t.is_contiguous() or t.data_ptr() % 16 != 0:
            return False
    return True


def relu(x):
    if not _hip_eligible(x):
        return torch.relu(x)
    return ReluFunction.apply(x)


def add(a, b):
    """Row-aligned sum of two feature matrices on ONE coordinate map (the BasicBlock residual).  Shapes must agree: a sparse add
    never broadcasts (a [N, C] + [1, C] would be a coordinate-map bug turned into numbers)."""
    if a.shape != b.shape:
        raise ValueError("add: feature matrices of shapes %s and %s (tensors on the same coordinate map have equal shapes)"
                         % (tuple(a.shape), tuple(b.shape)))
    if not _hip_eligible(a, b) and a.is_cuda and b.is_cuda:
        return a + b                    # dtype / stride / alignment the kernel does not take
    return AddFunction.apply(a, b)


def cat(ts):
    """Column concat of feature matrices on one coordinate map, left to right: one HIP launch per pair (the
    reference only ever concatenates two tensors).  Widths that are not multiples of 4, other dtypes and unaligned views
    take torch.cat on the device."""
    if all(t.is_cuda for t in ts) and (not _hip_eligible(*ts) or any(t.dim() != 2 or t.shape[1] % 4 or t.shape[1] < 4 for t in ts)):
        return torch.cat(list(ts), dim=1)
    out = ts[0]
    for t in ts[1:]:
        out = Cat2Function.apply(out, t)
    return out


def sparse_conv(feats, kernel, maps, n_out, tiles=None, counts=None, lists=None, transposed=False, fine_unique=False, training=True):
    """maps = CoordinateManager.kmap(...); tiles = .kmap_tiles(...) or None; counts = .kmap_counts(...) or None;
    lists = .kmap_lists(...) or None; transposed: the conv is a MinkowskiConvolutionTranspose; fine_unique: the map is a
    2^3 stride-2 map (every row of its fine side has exactly one pair); training: the calling module's mode -- an evaluation-mode
    convolution that records no graph runs in the inference precision in force, every other one in the training precision
    (openscene_amd.precision.pass_pieces), as the executor's pass does."""
    nbr_fwd, nbr_bwd, flip = maps
    grad = torch.is_grad_enabled() and (feats.requires_grad or kernel.requires_grad)
    pieces = precision.pass_pieces(training, grad)
    tf, tb = tiles if tiles is not None else (None, None)
    lf, lb = lists if lists is not None else (None, None)
    return SparseConvFunction.apply(feats, kernel, nbr_fwd, nbr_bwd, flip, n_out, tf, tb, counts, lf, lb, bool(transposed),
                                    bool(fine_unique), pieces)


_tls = threading.local()


class deferred_bn_counters:
    """Context: collect the `num_batches_tracked += 1` of every BN in a forward pass and apply them as ONE
    multi-tensor add at exit (48 one-element launches -> 1).  Same final buffer values as nn.BatchNorm1d.
    The pending list is per thread (two forwards on two threads do not see each other's counters)."""

    @staticmethod
    def current():
        return getattr(_tls, "pending", None)

    def __enter__(self):
        self.prev = getattr(_tls, "pending", None)
        _tls.pending = self.pending = []
        return self

    def __exit__(self, *exc):
        _tls.pending = self.prev
        if self.pending:
            torch._foreach_add_(self.pending, 1)
        return False


_relu_observer = None


def set_relu_observer(fn):
    """Test hook: `fn(y)` is called with the output of every fused BN(+residual)+ReLU, in call order
    (None switches it off).  Parity tests record the run's activation pattern through it."""
    global _relu_observer
    _relu_observer = fn


def batch_norm_act(x, bn, residual=None, relu=False):
    """`bn` is a torch.nn.BatchNorm1d (the `.bn` of MinkowskiBatchNorm): same parameters,
    buffers and train/eval semantics, computed by the HIP kernels."""
    training = bn.training or (bn.running_mean is None)
    momentum = 0.1 if bn.momentum is None else bn.momentum
    if bn.training and bn.track_running_stats and bn.num_batches_tracked is not None:
        if bn.momentum is None:                       # cumulative average: needs the count now (host sync)
            bn.num_batches_tracked.add_(1)
            momentum = 1.0 / float(bn.num_batches_tracked)
        elif deferred_bn_counters.current() is not None:
            deferred_bn_counters.current().append(bn.num_batches_tracked)
        else:
            bn.num_batches_tracked.add_(1)
    rm = bn.running_mean if bn.track_running_stats else None
    rv = bn.running_var if bn.track_running_stats else None
    if not training and rm is None:
        raise RuntimeError("eval-mode batch norm needs running statistics")
    gamma = bn.weight if bn.weight is not None else torch.ones(bn.num_features, device=x.device)
    beta = bn.bias if bn.bias is not None else torch.zeros(bn.num_features, device=x.device)
    y = BatchNormActFunction.apply(x, gamma, beta, rm, rv, residual, training, momentum, bn.eps, relu)
    if relu and _relu_observer is not None:
        _relu_observer(y)
    return y
