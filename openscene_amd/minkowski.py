"""The slice of the MinkowskiEngine Python surface that the reference touches,
re-implemented on the HIP kernels (SURVEY.md section 8(b) lists every symbol):

    import MinkowskiEngine as ME                          models/mink_unet.py:25
    from MinkowskiEngine.modules.resnet_block import BasicBlock, Bottleneck
    from MinkowskiEngine import SparseTensor              run/distill.py:18

``openscene_amd.install_minkowski_alias()`` registers this module under the
name ``MinkowskiEngine`` so those imports resolve unchanged.  Modules are plain
``nn.Module``s with ordinary ``nn.Parameter``s carrying ME's names and shapes
(``.kernel`` [K, Cin, Cout] -- 2-D [Cin, Cout] when K == 1 --, ``.bn`` =
``nn.BatchNorm1d``), so Adam, DDP, ``state_dict`` and the released checkpoints
work untouched.
"""
import math

import torch
import torch.nn as nn

from . import functional as F_
from .field import InterpolationMap, SparseTensorQuantizationMode, TensorField  # noqa: F401  (re-exported ME names)
from .sparse import ORIGIN_STRIDE, CoordinateManager, SparseTensor, cat  # noqa: F401  (re-exported ME names)

__version__ = "0.5.4+openscene_amd"


def _triple_ok(v, name):
    if isinstance(v, (list, tuple)):
        if len(set(v)) != 1:
            raise NotImplementedError("anisotropic %s %r is not used by the reference and not supported" % (name, v))
        v = v[0]
    return int(v)


class MinkowskiConvolutionBase(nn.Module):
    TRANSPOSED = False

    def __init__(self, in_channels, out_channels, kernel_size=-1, stride=1, dilation=1, bias=False,
                 kernel_generator=None, expand_coordinates=False, convolution_mode=None, dimension=None):
        super().__init__()
        if dimension is not None and dimension != 3:
            raise NotImplementedError("only 3-D sparse tensors are supported (dimension=%r)" % (dimension,))
        if kernel_generator is not None or expand_coordinates:
            raise NotImplementedError("custom kernel generators / coordinate expansion are outside the reference path")
        self.in_channels, self.out_channels = int(in_channels), int(out_channels)
        self.kernel_size = _triple_ok(kernel_size, "kernel_size")
        self.stride = _triple_ok(stride, "stride")
        self.dilation = _triple_ok(dilation, "dilation")
        if self.kernel_size < 1:
            raise ValueError("kernel_size must be >= 1")
        if self.stride not in (1, 2):
            raise NotImplementedError("stride %d: the reference only uses strides 1 and 2" % self.stride)
        self.dimension = 3
        self.kernel_volume = self.kernel_size ** 3
        shape = (self.in_channels, self.out_channels) if self.kernel_volume == 1 else \
            (self.kernel_volume, self.in_channels, self.out_channels)
        self.kernel = nn.Parameter(torch.empty(shape, dtype=torch.float32))
        self.bias = nn.Parameter(torch.empty(1, self.out_channels, dtype=torch.float32)) if bias else None
        self.reset_parameters()

    def reset_parameters(self):
        # ME default: U(-s, s), s = 1/sqrt(C * K), C = Cin (conv) or Cout (transposed)
        with torch.no_grad():
            n = (self.out_channels if self.TRANSPOSED else self.in_channels) * self.kernel_volume
            s = 1.0 / math.sqrt(n)
            self.kernel.uniform_(-s, s)
            if self.bias is not None:
                self.bias.uniform_(-s, s)

    def forward(self, x):
        cm, s_in = x.coordinate_manager, x.tensor_stride
        if self.TRANSPOSED:
            if self.stride == 1:
                # ME swaps the in/out maps of EVERY transposed conv (odd kernels: mirrored offsets); the reference
                # only builds stride-2 transposed convs (models/mink_unet.py:76-99), so refuse rather than return
                # the un-mirrored convolution silently
                raise NotImplementedError("MinkowskiConvolutionTranspose with stride 1 is outside the reference path")
            else:
                if s_in % self.stride:
                    raise ValueError("cannot up-sample a tensor of stride %d by %d" % (s_in, self.stride))
                s_out = s_in // self.stride
                if not cm.has(s_out):
                    raise RuntimeError("transposed convolution needs the cached stride-%d map of the encoder" % s_out)
        else:
            s_out = s_in * self.stride
        maps = cm.kmap(s_in, s_out, self.kernel_size, self.dilation)
        tiles = cm.kmap_tiles(s_in, s_out, self.kernel_size, self.dilation)
        counts = cm.kmap_counts(s_in, s_out, self.kernel_size, self.dilation) if self.kernel.requires_grad else None
        lists = None
        if F_.CONV_MODE == "tl" and self.kernel_volume > 1 and F_.ops.tl_eligible(self.kernel_volume, self.in_channels,
                                                                                  self.out_channels):
            lists = cm.kmap_lists(s_in, s_out, self.kernel_size, self.dilation)
        out = F_.sparse_conv(x.F, self.kernel, maps, cm.size(s_out), tiles, counts, lists, transposed=self.TRANSPOSED,
                             fine_unique=self.kernel_size == 2 and self.stride == 2 and self.dilation == 1, training=self.training)
        if self.bias is not None:
            out = out + self.bias
        return SparseTensor(out, tensor_stride=s_out, coordinate_manager=cm)

    def extra_repr(self):
        return "in=%d, out=%d, kernel_size=%d, stride=%d, dilation=%d" % (
            self.in_channels, self.out_channels, self.kernel_size, self.stride, self.dilation)


class MinkowskiConvolution(MinkowskiConvolutionBase):
    TRANSPOSED = False


class MinkowskiConvolutionTranspose(MinkowskiConvolutionBase):
    TRANSPOSED = True


class MinkowskiBatchNorm(nn.Module):
    """Holds ``self.bn = nn.BatchNorm1d`` exactly like ME (models/resnet_base.py:79-80
    initialises ``m.bn.weight``); the arithmetic runs in the HIP kernels."""

    def __init__(self, num_features, eps=1e-5, momentum=0.1, affine=True, track_running_stats=True):
        super().__init__()
        self.bn = nn.BatchNorm1d(num_features, eps=eps, momentum=momentum, affine=affine,
                                 track_running_stats=track_running_stats)

    def forward(self, x):
        return x._like(F_.batch_norm_act(x.F, self.bn))


class MinkowskiReLU(nn.Module):
    def __init__(self, inplace=False):
        super().__init__()
        self.inplace = inplace

    def forward(self, x):
        # stand-alone ReLU of the unfused module chain (fused paths: BasicBlock, openscene_amd.mink_unet)
        return x._like(F_.relu(x.F))


# ---- pooling, broadcast, linear (models/resnet_base.py:54,69,71; semantics recalled from ME v0.5.4) ----
class MinkowskiPoolingBase(nn.Module):
    """Parameter-free reduction over the kernel map of a convolution of the same geometry (the two share the cached map)."""
    MODE = None

    def __init__(self, kernel_size, stride=1, dilation=1, kernel_generator=None, expand_coordinates=False, dimension=None):
        super().__init__()
        if dimension is not None and dimension != 3:
            raise NotImplementedError("only 3-D sparse tensors are supported (dimension=%r)" % (dimension,))
        if kernel_generator is not None or expand_coordinates:
            raise NotImplementedError("custom kernel generators / coordinate expansion are outside the reference path")
        self.kernel_size = _triple_ok(kernel_size, "kernel_size")
        self.stride = _triple_ok(stride, "stride")
        self.dilation = _triple_ok(dilation, "dilation")
        if self.kernel_size not in (2, 3):
            raise NotImplementedError("pooling kernel_size %d: kernel sizes 2 and 3 are supported" % self.kernel_size)
        if self.stride not in (1, 2):
            raise NotImplementedError("stride %d: the reference only uses strides 1 and 2" % self.stride)
        self.dimension = 3
        self.kernel_volume = self.kernel_size ** 3

    def forward(self, x):
        cm, s_in = x.coordinate_manager, x.tensor_stride
        s_out = s_in * self.stride
        maps = cm.kmap(s_in, s_out, self.kernel_size, self.dilation)          # (ValueError on a globally pooled tensor)
        cnt = cm.pool_counts(s_in, s_out, self.kernel_size, self.dilation) if self.MODE == "avg" else None
        return SparseTensor(F_.local_pool(x.F, maps, self.MODE, cnt), tensor_stride=s_out, coordinate_manager=cm)

    def extra_repr(self):
        return "kernel_size=%d, stride=%d, dilation=%d" % (self.kernel_size, self.stride, self.dilation)


class MinkowskiSumPooling(MinkowskiPoolingBase):
    MODE = "sum"


class MinkowskiAvgPooling(MinkowskiPoolingBase):
    """Divides by the number of PRESENT inputs of an output voxel, not by the kernel volume."""
    MODE = "avg"


class MinkowskiMaxPooling(MinkowskiPoolingBase):
    MODE = "max"


class MinkowskiGlobalPoolingBase(nn.Module):
    """One output row per batch index present, in ascending batch index, on the input's coordinate manager; the result's
    tensor stride is sparse.ORIGIN_STRIDE and its coordinates are [[b, 0, 0, 0]]."""
    MODE = None

    def __init__(self, mode=None, dimension=None):
        super().__init__()
        if dimension is not None and dimension != 3:
            raise NotImplementedError("only 3-D sparse tensors are supported (dimension=%r)" % (dimension,))

    def forward(self, x):
        cm = x.coordinate_manager
        index = cm.batch_index(x.tensor_stride)
        return SparseTensor(F_.global_pool(x.F, index, self.MODE), tensor_stride=ORIGIN_STRIDE, coordinate_manager=cm)


class MinkowskiGlobalSumPooling(MinkowskiGlobalPoolingBase):
    MODE = "sum"


class MinkowskiGlobalAvgPooling(MinkowskiGlobalPoolingBase):
    MODE = "avg"


class MinkowskiGlobalMaxPooling(MinkowskiGlobalPoolingBase):
    MODE = "max"


class MinkowskiBroadcastBase(nn.Module):
    """forward(x, pooled): the pooled tensor's row of every row's batch, added to / multiplied with the row."""
    OP = None

    def forward(self, x, pooled):
        if pooled.coordinate_manager is not x.coordinate_manager or pooled.tensor_stride != ORIGIN_STRIDE:
            raise ValueError("broadcast: the second argument must be a globally pooled tensor of the first one's coordinate manager")
        index = x.coordinate_manager.batch_index(x.tensor_stride)
        return x._like(F_.broadcast(x.F, pooled.F, index, self.OP))


class MinkowskiBroadcastAddition(MinkowskiBroadcastBase):
    OP = "add"


class MinkowskiBroadcastMultiplication(MinkowskiBroadcastBase):
    OP = "mul"


class MinkowskiLinear(nn.Module):
    """Holds ``self.linear = nn.Linear`` exactly like ME (checkpoint keys ``linear.weight`` / ``linear.bias``).  Shapes the 1x1
    convolution kernel takes run on it (the K = 1 path of the convolutions, on ``linear.weight.t()``); every other shape runs
    torch.nn.functional.linear.  The bias is a row add."""

    def __init__(self, in_features, out_features, bias=True):
        super().__init__()
        self.linear = nn.Linear(in_features, out_features, bias=bias)

    def forward(self, x):
        lin, f = self.linear, x.F
        if (f.dtype == torch.float32 and lin.weight.dtype == torch.float32
                and F_.ops.dense_eligible(lin.in_features, lin.out_features)):
            out = F_.sparse_conv(f, lin.weight.t(), (None, None, False), f.shape[0], training=self.training)
            if lin.bias is not None:
                out = out + lin.bias
        else:
            out = nn.functional.linear(f, lin.weight, lin.bias)
        return x._like(out)


class MinkowskiInterpolation(nn.Module):
    """forward(input, positions): the features of `input` interpolated trilinearly at `positions` float [M, 4] (batch, x, y, z)
    in lattice units, a plain float32 [M, C] tensor -- SparseTensor.features_at_coordinates as a layer.  return_kernel_map /
    return_weights append this engine's own tables to the result: nbr int32 [8, M] (-1: absent) and w float32 [8, M], corner
    k = dx + 2 dy + 4 dz (ME returns its in / out map pair instead)."""

    def __init__(self, return_kernel_map=False, return_weights=False):
        super().__init__()
        self.return_kernel_map, self.return_weights = bool(return_kernel_map), bool(return_weights)

    def forward(self, input, positions):
        imap = InterpolationMap(input.coordinate_manager, input.tensor_stride, positions)
        out = F_.interpolate(input.F, imap)
        if not (self.return_kernel_map or self.return_weights):
            return out
        return (out,) + ((imap.nbr,) if self.return_kernel_map else ()) + ((imap.w,) if self.return_weights else ())


# ---- ME.modules.resnet_block ------------------------------------------------
class BasicBlock(nn.Module):
    """conv3-bn-relu-conv3-bn-(+residual)-relu, expansion 1 ([ME] modules/resnet_block.py;
    member names conv1/norm1/conv2/norm2/downsample are the checkpoint keys).  BN, the
    residual add and the ReLU run as ONE fused kernel pass per BN."""
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, dilation=1, downsample=None, bn_momentum=0.1, dimension=-1):
        super().__init__()
        self.conv1 = MinkowskiConvolution(inplanes, planes, kernel_size=3, stride=stride, dilation=dilation,
                                          dimension=dimension)
        self.norm1 = MinkowskiBatchNorm(planes, momentum=bn_momentum)
        self.conv2 = MinkowskiConvolution(planes, planes, kernel_size=3, stride=1, dilation=dilation,
                                          dimension=dimension)
        self.norm2 = MinkowskiBatchNorm(planes, momentum=bn_momentum)
        self.relu = MinkowskiReLU(inplace=True)
        self.downsample = downsample

    def forward(self, x):
        out = self.conv1(x)
        out = out._like(F_.batch_norm_act(out.F, self.norm1.bn, relu=True))
        out = self.conv2(out)
        if self.downsample is not None:
            ds = self.downsample
            if isinstance(ds, nn.Sequential) and len(ds) == 2 and isinstance(ds[1], MinkowskiBatchNorm):
                res = ds[0](x)
                res = F_.batch_norm_act(res.F, ds[1].bn)
            else:
                res = ds(x).F
        else:
            res = x.F
        return out._like(F_.batch_norm_act(out.F, self.norm2.bn, residual=res, relu=True))


class Bottleneck(nn.Module):
    """1x1 - 3x3x3 - 1x1 (expansion 4); imported by the reference, used by no shipped config."""
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, dilation=1, downsample=None, bn_momentum=0.1, dimension=-1):
        super().__init__()
        self.conv1 = MinkowskiConvolution(inplanes, planes, kernel_size=1, dimension=dimension)
        self.norm1 = MinkowskiBatchNorm(planes, momentum=bn_momentum)
        self.conv2 = MinkowskiConvolution(planes, planes, kernel_size=3, stride=stride, dilation=dilation,
                                          dimension=dimension)
        self.norm2 = MinkowskiBatchNorm(planes, momentum=bn_momentum)
        self.conv3 = MinkowskiConvolution(planes, planes * self.expansion, kernel_size=1, dimension=dimension)
        self.norm3 = MinkowskiBatchNorm(planes * self.expansion, momentum=bn_momentum)
        self.relu = MinkowskiReLU(inplace=True)
        self.downsample = downsample

    def forward(self, x):
        out = self.conv1(x)
        out = out._like(F_.batch_norm_act(out.F, self.norm1.bn, relu=True))
        out = self.conv2(out)
        out = out._like(F_.batch_norm_act(out.F, self.norm2.bn, relu=True))
        out = self.conv3(out)
        res = self.downsample(x).F if self.downsample is not None else x.F
        return out._like(F_.batch_norm_act(out.F, self.norm3.bn, residual=res, relu=True))


# ---- ME.utils ------------------------------------------------------------------
def kaiming_normal_(tensor, a=0, mode="fan_in", nonlinearity="leaky_relu"):
    """ME.utils.kaiming_normal_ (models/resnet_base.py:76): fan_in = Cin*K, fan_out = Cout*K for a
    [K, Cin, Cout] kernel (plain [Cin, Cout] when K == 1)."""
    if tensor.dim() == 3:
        k, cin, cout = tensor.shape
    elif tensor.dim() == 2:
        k, (cin, cout) = 1, tensor.shape
    else:
        raise ValueError("kernel tensors are [K, Cin, Cout] or [Cin, Cout]")
    fan = cin * k if mode == "fan_in" else cout * k
    gain = nn.init.calculate_gain(nonlinearity, a)
    std = gain / math.sqrt(fan)
    with torch.no_grad():
        return tensor.normal_(0, std)


def batched_coordinates(coords, dtype=torch.int32, device=None):
    """ME.utils.batched_coordinates: a list of [N_i, 3] coordinate arrays or tensors -> [sum N_i, 4] rows (batch, x, y, z), the
    batch index = the position in the list.  dtype torch.int32 (voxels) or a floating dtype (a TensorField's positions)."""
    rows = []
    for b, c in enumerate(coords):
        c = torch.as_tensor(c)
        if c.dim() != 2 or c.shape[1] != 3:
            raise ValueError("batched_coordinates: entry %d has shape %s, expected [N, 3]" % (b, tuple(c.shape)))
        c = (torch.floor(c) if c.dtype.is_floating_point and not dtype.is_floating_point else c).to(dtype)
        rows.append(torch.cat([torch.full((c.shape[0], 1), b, dtype=dtype, device=c.device), c], 1))
    out = torch.cat(rows, 0) if rows else torch.zeros((0, 4), dtype=dtype)
    return out if device is None else out.to(device)


def sparse_collate(coords, feats, dtype=torch.int32, device=None):
    """ME.utils.sparse_collate without labels: (batched_coordinates(coords), the feature matrices stacked in the same order)."""
    if len(coords) != len(feats):
        raise ValueError("sparse_collate: %d coordinate lists vs %d feature matrices" % (len(coords), len(feats)))
    for b, (c, f) in enumerate(zip(coords, feats)):
        if len(c) != len(f):
            raise ValueError("sparse_collate: entry %d has %d coordinates and %d feature rows" % (b, len(c), len(f)))
    f = torch.cat([torch.as_tensor(v) for v in feats], 0) if len(feats) else torch.zeros((0, 0))
    return batched_coordinates(coords, dtype=dtype, device=device), (f if device is None else f.to(device))
