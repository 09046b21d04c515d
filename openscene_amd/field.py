"""TensorField: points in, points out ([ME] TensorField, SparseTensorQuantizationMode, MinkowskiInterpolation's map).

The networks of this package take voxels and return voxels; the points live outside them.  The reference's evaluation hands a
point the row of the voxel it fell into (run/evaluate.py:283-292: ``SparseTensor(feat, coords)`` on the voxeliser's unique rows,
then ``predictions[inds_reverse]``).  A field keeps the points themselves:

    field = TensorField(point_features, positions / voxel_size)      # float32 [N, C], float32 [N, 4] rows (batch, x, y, z)
    x = field.sparse()                                               # voxels: the AVERAGE of every voxel's points
    out = net(x)
    out.slice(field).F                                               # == out.F[field.inverse_mapping]: the row of a point's voxel
    out.interpolate(field).F                                         # trilinear between the eight voxels around every point

Every step is differentiable in the features (never in the positions) and bit for bit repeatable: no floating-point atomics.
Semantics are recalled from MinkowskiEngine v0.5.4 and restated in DESIGN.md section 4; tests/field_reference.py is that
section in numpy.
"""
import enum

import torch

from . import functional as F_
from . import ops
from .sparse import ORIGIN_STRIDE, CoordinateManager, SparseTensor


class SparseTensorQuantizationMode(enum.Enum):
    """What the feature row of a voxel is when several rows share its coordinates."""
    RANDOM_SUBSAMPLE = 0          # the first row in the caller's order (what SparseTensor always did, and still defaults to)
    UNWEIGHTED_AVERAGE = 1        # the ordered fp32 sum divided by the number of rows (a TensorField's default)
    UNWEIGHTED_SUM = 2            # the fp32 sum of the rows in ascending row index, added one by one from +0
    MAX_POOL = 4                  # not implemented


_MODE_WORD = {SparseTensorQuantizationMode.RANDOM_SUBSAMPLE: "first", SparseTensorQuantizationMode.UNWEIGHTED_AVERAGE: "avg",
              SparseTensorQuantizationMode.UNWEIGHTED_SUM: "sum"}


def mode_word(mode, default):
    """The functional.quantize word of a SparseTensorQuantizationMode (None: `default`)."""
    mode = default if mode is None else mode
    if not isinstance(mode, SparseTensorQuantizationMode):
        raise TypeError("quantization_mode must be a SparseTensorQuantizationMode (got %r)" % (mode,))
    if mode not in _MODE_WORD:
        raise NotImplementedError("quantization mode %s is not implemented (sum, average and subsample are)" % mode.name)
    return _MODE_WORD[mode]


def quantize_positions(positions):
    """float32 [N, 4] positions -> int32 [N, 4] cells: floorf of every float32 value.  A non-finite value, a batch outside
    [0, 65535) or a cell outside (-32767, 32767) is a ValueError; finding out costs one host read."""
    p = positions
    lim = 32767.0
    cells = torch.floor(p)
    ok = torch.isfinite(p).all() & (cells[:, 1:].abs() < lim).all() & (cells[:, 0] >= 0).all() & (cells[:, 0] < 65535.0).all()
    if not bool(ok):
        raise ValueError("TensorField: a position is not finite or outside the packable range "
                         "(|x|,|y|,|z| < 32767, 0 <= batch < 65535)")
    return cells.int()


class InterpolationMap:
    """The corners and weights of `positions` float32 [M, 4] in the stride's map of a manager: nbr int32 [8, M] (-1: absent),
    w float32 [8, M], corner k = dx + 2 dy + 4 dz.  `.invalid` counts the rows that have no cell (not finite, batch or cell out
    of range); it lives on the device and is read -- one synchronisation -- only when asked.  The backward plan is built on the
    first backward pass through the map and kept."""

    def __init__(self, manager, stride, positions):
        if stride == ORIGIN_STRIDE or not manager.has(stride):
            raise ValueError("interpolation needs a spatial tensor of this coordinate manager (tensor stride %r)" % (stride,))
        manager.coords(stride)
        self.stride = stride
        self.n_in = manager.size(stride)
        self.nbr, self.w, self._bad = ops.field_map(manager._tables[stride], positions, stride)
        self._plan = None

    @property
    def invalid(self):
        return int(self._bad)

    def plan(self):
        if self._plan is None:
            self._plan = ops.interp_plan(self.nbr, self.n_in)
        return self._plan


class TensorField:
    """features float32 [N, C] at coordinates float32 [N, 4] (batch, x, y, z), positions in lattice units: divide by the voxel
    size first, as with ME.  The batch column holds an integral value.  Coordinates of another floating dtype are converted
    with ``.float()`` (the reference's voxeliser floors float64 values: a point within one float32 ulp of a cell wall may land
    on the other side); integer coordinates are taken as they are.  `device`: where to move both first.

    ``.sparse()`` quantises: the cell of a point is floorf of its position, the voxel rows come in first-occurrence order, and
    `quantization_mode` (default UNWEIGHTED_AVERAGE) says what a voxel's row is.  The coordinate manager, ``inverse_mapping``
    and the voxels' point lists are built on first use -- one host read for the range check, the manager's own for its sizes --
    and kept, so ``slice`` / ``interpolate`` of any tensor the network derives from ``.sparse()`` find them."""

    def __init__(self, features, coordinates, quantization_mode=SparseTensorQuantizationMode.UNWEIGHTED_AVERAGE,
                 device=None):
        if device is not None:
            features, coordinates = features.to(device), coordinates.to(device)
        if coordinates.dim() != 2 or coordinates.shape[1] != 4:
            raise ValueError("TensorField coordinates must be [N, 4] rows (batch, x, y, z), got %s" % (tuple(coordinates.shape),))
        if coordinates.shape[0] != features.shape[0]:
            raise ValueError("%d feature rows vs %d coordinate rows" % (features.shape[0], coordinates.shape[0]))
        if coordinates.device != features.device:
            raise ValueError("features on %s but coordinates on %s" % (features.device, coordinates.device))
        mode_word(quantization_mode, None)                # (refuses MAX_POOL here, not at the first .sparse())
        self._F = features
        self._C = coordinates.float().contiguous()
        self.quantization_mode = quantization_mode
        self._manager = None
        self._imaps = {}

    # ME names
    @property
    def F(self):
        return self._F

    @property
    def C(self):
        return self._C

    features = F
    coordinates = C

    @property
    def device(self):
        return self._F.device

    @property
    def shape(self):
        return self._F.shape

    def __len__(self):
        return self._F.shape[0]

    @property
    def coordinate_manager(self):
        if self._manager is None:
            self._manager = CoordinateManager(quantize_positions(self._C))
        return self._manager

    @property
    def inverse_mapping(self):
        """int64 [N]: the row of every point's voxel in ``.sparse()``."""
        return self.coordinate_manager.point_index(1).rank.long()

    def _like(self, features):
        f = TensorField.__new__(TensorField)
        f._F, f._C, f.quantization_mode, f._manager, f._imaps = features, self._C, self.quantization_mode, self._manager, self._imaps
        return f

    def sparse(self, tensor_stride=1, quantization_mode=None):
        """The field's voxels as a SparseTensor on the field's coordinate manager (created here, shared with nothing else)."""
        if tensor_stride != 1:
            raise ValueError("TensorField.sparse: tensor_stride %r (a field quantises to stride 1)" % (tensor_stride,))
        word = mode_word(quantization_mode, self.quantization_mode)
        cm = self.coordinate_manager
        return SparseTensor(F_.quantize(self._F, cm.point_index(1), word), tensor_stride=1, coordinate_manager=cm)

    def point_index(self, tensor):
        """The PointIndex of `tensor`'s rows over this field's points; ValueError unless the tensor lives on the field's manager."""
        if self._manager is None or tensor.coordinate_manager is not self._manager:
            raise ValueError("slice: the tensor does not live on the coordinate manager this field created with .sparse()")
        if tensor.tensor_stride == ORIGIN_STRIDE or not self._manager.has(tensor.tensor_stride):
            raise ValueError("slice: tensor stride %r is not a spatial map of the field's manager" % (tensor.tensor_stride,))
        return self._manager.point_index(tensor.tensor_stride)

    def interpolation_map(self, tensor):
        """The InterpolationMap of this field's positions in `tensor`'s map (kept per stride for the field's own manager)."""
        cm, s = tensor.coordinate_manager, tensor.tensor_stride
        if cm is not self._manager:
            return InterpolationMap(cm, s, self._C)
        if s not in self._imaps:
            self._imaps[s] = InterpolationMap(cm, s, self._C)
        return self._imaps[s]

    def __repr__(self):
        return "TensorField(N=%d, C=%d, %s, device=%s)" % (self._F.shape[0], self._F.shape[1], self.quantization_mode.name, self._F.device)
