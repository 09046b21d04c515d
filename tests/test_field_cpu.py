"""TensorField, slice and trilinear interpolation without a GPU: the laws of the numpy restatement the GPU tests compare against
(tests/field_reference.py), the MinkowskiEngine names and defaults, the module tree on the CPU backend (gradients against
float64, how many C-level calls a pass makes), and the argument checks of every new C entry."""
import ctypes
import os

import numpy as np
import pytest
import torch

import cpu_backend
import field_reference as fr
from oracle import coords as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
EPS = 2.0 ** -24


def cloud(seed, n=300, side=5.0, batches=2, dyadic=False):
    """float32 [n, 4] positions (batch, x, y, z), negative ones included; dyadic: multiples of 1/4."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-side, side, (n, 3))
    if dyadic:
        p = np.round(p * 4) / 4
    return np.concatenate([rng.integers(0, batches, (n, 1)).astype(np.float64), p], 1).astype(F32)


# ---- the restatement's own laws ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [1, 2, 4])
def test_table_of_the_restatement_is_the_kernel_map_of_the_base_cells(s):
    pos = cloud(0)
    uniq, inv, _, _ = fr.quantize_map(pos)
    coords_s, _ = fr.strided_inverse(uniq, inv, s)
    extra = np.array([[0, -0.25, 0.5, 1.0], [1, 3.0, -4.0, 2.0], [0, np.nan, 0, 0], [0, np.inf, 0, 0], [-1, 0, 0, 0],
                      [65535, 0, 0, 0], [0, 40000.3, 0, 0]], F32)
    pos = np.concatenate([pos, extra])
    nbr, w, bad, t, valid = fr.interp_map(coords_s, pos, s)
    assert bad == 5 and valid[:-5].all() and not valid[-5:].any()
    assert (nbr[:, ~valid] == -1).all() and (w[:, ~valid] == 0).all() and not np.signbit(w[:, ~valid]).any()
    _, batch, base, _ = fr.interp_geometry(pos, s)
    rows = np.concatenate([batch[:, None], base], 1)[valid].astype(np.int32)
    assert np.array_equal(nbr[:, valid], oc.kernel_map(coords_s, rows, oc.kernel_offsets(2, s)))
    assert (nbr[:, valid] >= 0).any() and (nbr[:, valid] < 0).any()
    # -0.25 floors to -1 (stride 4: base -4), never truncates to 0
    assert base[len(pos) - 7, 0] == -s and t[len(pos) - 7, 0] == F32(-0.25) / F32(s) + F32(1)


def test_partition_of_unity_inside_a_solid_block():
    g = np.stack(np.meshgrid(*[np.arange(4)] * 3, indexing="ij"), -1).reshape(-1, 3)
    coords = np.concatenate([np.zeros((64, 1), np.int32), g.astype(np.int32)], 1)
    rng = np.random.default_rng(1)
    pos = np.concatenate([np.zeros((200, 1)), rng.uniform(0, 3, (200, 3))], 1).astype(F32)
    nbr, w, bad, t, valid = fr.interp_map(coords, pos, 1)
    assert bad == 0 and (nbr >= 0).all()
    for const in (1.0, -3.7):
        y = fr.interp_fwd(np.full((64, 2), const, F32), nbr, w)
        y64, s64 = fr.interp_fwd64(np.full((64, 2), F32(const)), nbr, fr.weights64(t, valid))
        assert np.allclose(y64, F32(const), rtol=0, atol=1e-12)              # the exact weights sum to one
        assert (np.abs(y - y64) <= 12 * EPS * s64).all()


@pytest.mark.parametrize("s", [1, 2])
def test_backward_is_the_transpose_of_forward_exactly_on_dyadic_operands(s):
    """<gy, I x> = <I^T gy, x>: integer-valued x and gy, t a multiple of 1/4 -- every product and sum is exact."""
    pos = cloud(2, dyadic=True)
    if s == 2:
        pos[:, 1:] *= 2                                                       # t = q - floor(q) stays a multiple of 1/4
    uniq, inv, _, _ = fr.quantize_map(pos)
    coords_s, _ = fr.strided_inverse(uniq, inv, s)
    nbr, w, _, _, _ = fr.interp_map(coords_s, pos, s)
    rng = np.random.default_rng(3)
    x = rng.integers(-8, 9, (coords_s.shape[0], 5)).astype(F32)
    gy = rng.integers(-8, 9, (pos.shape[0], 5)).astype(F32)
    y, gx = fr.interp_fwd(x, nbr, w), fr.interp_bwd(gy, nbr, w, coords_s.shape[0])
    assert float((gy.astype(np.float64) * y).sum()) == float((gx.astype(np.float64) * x).sum())
    assert np.abs(gx).sum() > 0


def test_a_point_on_a_lattice_site_returns_the_voxel_row_bit_for_bit():
    coords = np.array([[0, 1, 2, 3], [0, -4, 0, 8]], np.int32)
    x = np.random.default_rng(4).standard_normal((2, 3)).astype(F32)
    nbr, w, _, _, _ = fr.interp_map(coords[:1], np.array([[0, 1, 2, 3]], F32), 1)
    assert np.array_equal(fr.interp_fwd(x[:1], nbr, w).view(np.int32), x[:1].view(np.int32))
    nbr, w, _, _, _ = fr.interp_map(coords[1:], np.array([[0, -4, 0, 8]], F32), 4)
    assert nbr[0, 0] == 0 and np.array_equal(fr.interp_fwd(x[1:], nbr, w).view(np.int32), x[1:].view(np.int32))


def test_quantisation_against_the_dense_float64_operator():
    pos = cloud(5, n=400, side=2.0)
    uniq, inv, first, cnt = fr.quantize_map(pos)
    Q = fr.quantize_dense(pos)
    assert Q.shape == (uniq.shape[0], 400) and np.array_equal(Q.sum(1), cnt) and cnt.max() > 1
    assert np.array_equal(np.argmax(Q, 1), first) and np.array_equal(np.argmax(Q, 0), inv)          # first-occurrence order
    rng = np.random.default_rng(6)
    x = rng.standard_normal((400, 4)).astype(F32)
    lim = cnt[:, None] * EPS * (Q @ np.abs(x.astype(np.float64)))
    assert (np.abs(fr.quantize_fwd(x, inv, first, cnt, "sum") - Q @ x.astype(np.float64)) <= lim).all()
    assert (np.abs(fr.quantize_fwd(x, inv, first, cnt, "avg") - Q @ x.astype(np.float64) / cnt[:, None]) <= lim).all()
    assert np.array_equal(fr.quantize_fwd(x, inv, first, cnt, "first"), x[first])
    xi = rng.integers(-8, 9, (400, 4)).astype(F32)
    assert np.array_equal(fr.quantize_fwd(xi, inv, first, cnt, "sum"), (Q @ xi.astype(np.float64)).astype(F32))
    gy = rng.standard_normal((uniq.shape[0], 4)).astype(F32)
    assert np.array_equal(fr.quantize_bwd(gy, inv, first, cnt, "sum"), (Q.T @ gy.astype(np.float64)).astype(F32))
    assert np.array_equal(fr.quantize_bwd(gy, inv, first, cnt, "avg"), gy[inv] / cnt.astype(F32)[inv][:, None])
    gf = fr.quantize_bwd(gy, inv, first, cnt, "first")
    assert np.array_equal(gf[first], gy) and np.count_nonzero(gf.any(1)) <= uniq.shape[0]


@pytest.mark.parametrize("const", [1.5, -0.375])
def test_the_average_of_a_constant_is_the_constant(const):
    """k * const is exact for every k <= 27, so the one division gives the constant back bit for bit."""
    inv = np.concatenate([np.full(k, k - 1) for k in range(1, 28)])
    cnt = np.arange(1, 28)
    first = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    x = np.full((inv.shape[0], 3), const, F32)
    y = fr.quantize_fwd(x, inv, first, cnt, "avg")
    assert np.array_equal(y.view(np.int32), np.full_like(y, const).view(np.int32))


# ---- ME names -----------------------------------------------------------------------------------------------------------------------
def test_me_names_and_defaults():
    import inspect
    import openscene_amd
    from openscene_amd import minkowski as mk
    me = openscene_amd.install_minkowski_alias()
    for name in ("TensorField", "SparseTensorQuantizationMode", "MinkowskiInterpolation", "SparseTensor"):
        assert getattr(me, name) is getattr(mk, name)
    assert openscene_amd.TensorField is mk.TensorField and openscene_amd.MinkowskiInterpolation is mk.MinkowskiInterpolation
    assert openscene_amd.SparseTensorQuantizationMode is mk.SparseTensorQuantizationMode and openscene_amd.InterpolationMap is mk.InterpolationMap
    assert me.utils.batched_coordinates is mk.batched_coordinates and me.utils.sparse_collate is mk.sparse_collate
    Q = mk.SparseTensorQuantizationMode
    assert {"RANDOM_SUBSAMPLE", "UNWEIGHTED_AVERAGE", "UNWEIGHTED_SUM", "MAX_POOL"} <= set(Q.__members__)
    assert inspect.signature(mk.TensorField.__init__).parameters["quantization_mode"].default is Q.UNWEIGHTED_AVERAGE     # the field averages
    assert inspect.signature(mk.SparseTensor.__init__).parameters["quantization_mode"].default is None                   # the tensor subsamples
    for m in ("slice", "cat_slice", "interpolate", "features_at_coordinates"):
        assert callable(getattr(mk.SparseTensor, m))
    layer = mk.MinkowskiInterpolation()
    assert not layer.return_kernel_map and not layer.return_weights and not list(layer.parameters())
    f, c = torch.ones(2, 3), torch.zeros(2, 4)
    with pytest.raises(NotImplementedError):
        mk.TensorField(f, c, quantization_mode=Q.MAX_POOL)
    with pytest.raises(NotImplementedError):
        mk.TensorField(f, c).sparse(quantization_mode=Q.MAX_POOL)
    with pytest.raises(ValueError):
        mk.TensorField(f, c).sparse(tensor_stride=2)
    with pytest.raises(ValueError):
        mk.TensorField(f, c[:, :3])
    with pytest.raises(NotImplementedError):
        mk.SparseTensor(f, c.int(), quantization_mode=Q.MAX_POOL)


def test_utils_batch_coordinates_and_collate():
    from openscene_amd import minkowski as mk
    a, b = np.array([[1, 2, 3], [4, 5, 6]]), torch.tensor([[7, 8, 9]])
    bc = mk.batched_coordinates([a, b])
    assert bc.dtype == torch.int32 and bc.tolist() == [[0, 1, 2, 3], [0, 4, 5, 6], [1, 7, 8, 9]]
    fc = mk.batched_coordinates([a * 0.5, b.float()], dtype=torch.float32)
    assert fc.dtype == torch.float32 and fc[1].tolist() == [0.0, 2.0, 2.5, 3.0] and fc[2, 0] == 1
    assert mk.batched_coordinates([np.array([[-0.5, 0.5, 1.5]])]).tolist() == [[0, -1, 0, 1]]            # floor, not truncation
    c, f = mk.sparse_collate([a, b], [torch.ones(2, 4), torch.zeros(1, 4)])
    assert c.shape == (3, 4) and f.shape == (3, 4) and f[:, 0].tolist() == [1, 1, 0]
    with pytest.raises(ValueError):
        mk.sparse_collate([a, b], [torch.ones(2, 4)])
    with pytest.raises(ValueError):
        mk.batched_coordinates([np.zeros((2, 4))])


# ---- the module tree on the CPU backend -----------------------------------------------------------------------------------------
def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def cpu_field_map(table, positions, stride):
    nbr, w, bad, _, _ = fr.interp_map(table.coords4, positions.detach().numpy(), int(stride))
    return _t(nbr), _t(w), torch.tensor([bad], dtype=torch.int32)


def cpu_interp_fwd(x, nbr, w):
    return _t(fr.interp_fwd(x.detach().numpy(), nbr.numpy(), w.numpy()))


def cpu_interp_bwd(gy, plan, w, n_in):
    """Evaluated FROM THE PLAN (not from the table), so the host-built lists are what is exercised."""
    pair, offsets = plan.pair.numpy().astype(np.int64), plan.offsets.numpy()
    m = gy.shape[0]
    seg = np.repeat(np.arange(n_in), np.diff(offsets))
    terms = (w.numpy().reshape(-1)[pair][:, None] * gy.detach().numpy()[pair % max(m, 1)]).astype(F32)
    assert np.array_equal(np.argsort(seg, kind="stable"), np.arange(seg.shape[0]))
    return _t(fr.ordered_sum(terms, seg, n_in))


def cpu_segment_reduce(x, order, offsets, mode):
    order, offsets = order.numpy().astype(np.int64), offsets.numpy()
    n_seg = offsets.shape[0] - 1
    seg = np.empty(order.shape[0], np.int64)
    seg[order] = np.repeat(np.arange(n_seg), np.diff(offsets))
    for u in range(n_seg):                                                 # ascending point index inside every list
        assert (np.diff(order[offsets[u]:offsets[u + 1]]) > 0).all()
    y = fr.ordered_sum(x.detach().numpy(), seg, n_seg)
    if mode == "avg":
        y = y / np.diff(offsets).astype(F32)[:, None]
    return _t(y)


def cpu_segment_expand(g, rank, offsets=None, mode="sum"):
    y = g.detach().numpy()[rank.numpy().astype(np.int64)]
    if mode == "avg":
        y = y / np.diff(offsets.numpy()).astype(F32)[rank.numpy().astype(np.int64)][:, None]
    return _t(y)


@pytest.fixture()
def cpu_ops(monkeypatch):
    """tests/cpu_backend.py swapped in for openscene_amd.ops, the CPU forms of the new functions attached to it, every one counted."""
    from openscene_amd import ops
    cpu_backend.install(monkeypatch)
    calls = {}

    def counted(name, fn):
        def wrapped(*a, **kw):
            calls[name] = calls.get(name, 0) + 1
            return fn(*a, **kw)
        return wrapped
    for name, fn in (("field_map", cpu_field_map), ("interp_fwd", cpu_interp_fwd), ("interp_bwd", cpu_interp_bwd),
                     ("segment_reduce", cpu_segment_reduce), ("segment_expand", cpu_segment_expand), ("interp_plan", ops.interp_plan)):
        monkeypatch.setattr(ops, name, counted(name, fn))
    return calls


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def test_module_tree_on_the_cpu_backend(cpu_ops):
    from openscene_amd import minkowski as mk
    pos = cloud(7, n=500, side=3.0)
    torch.manual_seed(0)
    feats = torch.randn(500, 3, requires_grad=True)
    conv1 = mk.MinkowskiConvolution(3, 8, kernel_size=3, dimension=3)
    conv2 = mk.MinkowskiConvolution(8, 8, kernel_size=2, stride=2, dimension=3)
    field = mk.TensorField(feats, _t(pos))
    x = field.sparse()
    assert x.coordinate_manager is field.coordinate_manager and x.tensor_stride == 1 and x.shape[0] < 500
    out = conv2(conv1(x))
    y = out.interpolate(field)
    assert isinstance(y, mk.TensorField) and y.F.shape == (500, 8) and y.C is field.C
    y.F.square().sum().backward()
    f64 = feats.detach().double().requires_grad_(True)
    w1, w2 = conv1.kernel.detach().double().requires_grad_(True), conv2.kernel.detach().double().requires_grad_(True)
    y64, h64, x64 = fr.chain64(f64, pos, w1, w2)
    y64.square().sum().backward()
    assert rel(y.F.detach(), y64.detach()) < 1e-5 and rel(x.F.detach(), x64.detach()) < 1e-6
    assert rel(feats.grad, f64.grad) < 1e-5 and rel(conv1.kernel.grad, w1.grad) < 1e-5 and rel(conv2.kernel.grad, w2.grad) < 1e-5
    # one reduce for the quantisation and one gather for its backward; one map, one forward, one plan and one backward
    assert cpu_ops == dict(segment_reduce=1, segment_expand=1, field_map=1, interp_fwd=1, interp_plan=1, interp_bwd=1), cpu_ops
    # a second pass over the same field builds nothing again: the map and its plan are kept
    cpu_ops.clear()
    torch.autograd.grad(out.interpolate(field).F.sum(), out.F)
    assert cpu_ops == dict(interp_fwd=1, interp_bwd=1), cpu_ops
    # slice: the row of every point's voxel, at both strides; its backward is the ordered sum
    cpu_ops.clear()
    h = conv1(x)
    s1, s2 = h.slice(field), out.slice(field)
    assert torch.equal(s1.F, h.F[field.inverse_mapping]) and field.inverse_mapping.dtype == torch.int64
    rank2 = field.coordinate_manager.point_index(2).rank.long()
    assert torch.equal(out.C[rank2][:, 1:], torch.div(x.C[field.inverse_mapping][:, 1:], 2, rounding_mode="floor") * 2)
    assert torch.equal(out.C[rank2][:, 0], x.C[field.inverse_mapping][:, 0]) and torch.equal(s2.F, out.F[rank2])
    g = torch.autograd.grad(s2.F.sum(), out.F)[0]
    assert torch.equal(g, field.coordinate_manager.point_index(2).cnt.float()[:, None].expand_as(g))
    assert cpu_ops == dict(segment_expand=2, segment_reduce=1), cpu_ops
    assert h.cat_slice(field).F.shape == (500, 11) and torch.equal(h.cat_slice(field).F[:, 8:], feats)
    # another manager is refused, and so is a field that never made one
    other = mk.TensorField(feats.detach(), _t(pos))
    with pytest.raises(ValueError):
        out.slice(other)
    other.sparse()
    with pytest.raises(ValueError):
        out.slice(other)
    # positions that are not the field's own, through the layer and through the method
    q = _t(cloud(8, n=40, side=3.0))
    layer = mk.MinkowskiInterpolation(return_kernel_map=True, return_weights=True)
    yq, nbr, w = layer(out, q)
    assert yq.shape == (40, 8) and nbr.shape == (8, 40) and w.dtype == torch.float32
    assert torch.equal(yq, out.features_at_coordinates(q)) and torch.equal(mk.MinkowskiInterpolation()(out, q), yq)
    assert mk.InterpolationMap(out.coordinate_manager, 2, q).invalid == 0
    bad = mk.InterpolationMap(out.coordinate_manager, 2, torch.tensor([[0, float("nan"), 0, 0], [0, 40000.3, 0, 0], [0, 0.5, 0.5, 0.5]]))
    assert bad.invalid == 2


def test_quantisation_modes_of_fields_and_tensors(cpu_ops):
    from openscene_amd import minkowski as mk
    Q = mk.SparseTensorQuantizationMode
    pos = cloud(9, n=200, side=1.5)
    uniq, inv, first, cnt = fr.quantize_map(pos)
    feats = torch.randn(200, 5, generator=torch.Generator().manual_seed(1))
    for mode, word in ((None, "avg"), (Q.UNWEIGHTED_AVERAGE, "avg"), (Q.UNWEIGHTED_SUM, "sum"), (Q.RANDOM_SUBSAMPLE, "first")):
        f = feats.clone().requires_grad_(True)
        x = mk.TensorField(f, _t(pos)).sparse(quantization_mode=mode)
        assert np.array_equal(x.C.numpy(), uniq)
        assert np.array_equal(x.F.detach().numpy(), fr.quantize_fwd(feats.numpy(), inv, first, cnt, word))
        gy = torch.randn(x.shape, generator=torch.Generator().manual_seed(2))
        x.F.backward(gy)
        assert np.array_equal(f.grad.numpy(), fr.quantize_bwd(gy.numpy(), inv, first, cnt, word))
    # integer coordinates with duplicates: the default keeps the first row, the keyword is no longer swallowed
    ci = _t(fr.cells(pos))
    assert torch.equal(mk.SparseTensor(feats, ci).F, feats[_t(first)])
    assert torch.equal(mk.SparseTensor(feats, ci, quantization_mode=Q.RANDOM_SUBSAMPLE).F, feats[_t(first)])
    assert np.array_equal(mk.SparseTensor(feats, ci, quantization_mode=Q.UNWEIGHTED_SUM).F.numpy(),
                          fr.quantize_fwd(feats.numpy(), inv, first, cnt, "sum"))
    assert np.array_equal(mk.SparseTensor(feats, ci, quantization_mode=Q.UNWEIGHTED_AVERAGE).F.numpy(),
                          fr.quantize_fwd(feats.numpy(), inv, first, cnt, "avg"))
    # a field of a float64 dtype is converted; a position out of range or not finite is refused
    assert mk.TensorField(feats, _t(pos).double()).C.dtype == torch.float32
    for bad in ([0, float("nan"), 0, 0], [0, float("inf"), 0, 0], [-1, 0, 0, 0], [65535, 0, 0, 0], [0, 40000.3, 0, 0]):
        with pytest.raises(ValueError):
            mk.TensorField(torch.ones(1, 2), torch.tensor([bad], dtype=torch.float32)).sparse()


# ---- argument checks of the C entries: -1 (OSN_E_ARG), the entry's name first, nothing launched ------------------------------
def test_field_entries_argument_errors():
    import __graft_entry__ as ge
    ge.build()
    from openscene_amd import _lib, ops
    h = _lib.load()
    assert ops.SEGMENT_MODES == ("sum", "avg") and ops.POOL_MODES[:2] == ops.SEGMENT_MODES
    buf = (ctypes.c_char * (8192 + 16))()
    p = (ctypes.addressof(buf) + 15) & ~15
    a0, a1, a2, a3, a4, a5 = p, p + 1024, p + 2048, p + 3072, p + 4096, p + 5120
    n, c, cap = 8, 16, 1024

    def refused(name, rc):
        assert rc == -1, (name, rc)
        assert _lib.last_error().startswith(name + ":"), _lib.last_error()

    def fmap(**kw):
        a = dict(keys=a0, vals=a1, cap=cap, pos=a2, m=n, stride=1, nbr=a3, w=a4, bad=a5)
        a.update(kw)
        return h.osn_field_map(a["keys"], a["vals"], a["cap"], a["pos"], a["m"], a["stride"], a["nbr"], a["w"], a["bad"], None)
    for bad in (dict(keys=None), dict(vals=None), dict(pos=None), dict(nbr=None), dict(w=None), dict(bad=None), dict(stride=0), dict(stride=-2),
                dict(m=-1), dict(m=ops.FIELD_MAX_POINTS + 1), dict(cap=1000), dict(cap=0)):
        refused("osn_field_map", fmap(**bad))

    def ifwd(**kw):
        a = dict(x=a0, n_in=n, nbr=a1, w=a2, m=n, c=c, y=a3)
        a.update(kw)
        return h.osn_interp_fwd(a["x"], a["n_in"], a["nbr"], a["w"], a["m"], a["c"], a["y"], None)
    for bad in (dict(x=None), dict(nbr=None), dict(w=None), dict(y=None), dict(c=0), dict(c=-4), dict(m=-1), dict(n_in=-1),
                dict(m=ops.FIELD_MAX_POINTS + 1)):
        refused("osn_interp_fwd", ifwd(**bad))

    def ibwd(**kw):
        a = dict(gy=a0, m=n, c=c, pair=a1, n_pair=4, offsets=a2, w=a3, n_in=n, gx=a4)
        a.update(kw)
        return h.osn_interp_bwd(a["gy"], a["m"], a["c"], a["pair"], a["n_pair"], a["offsets"], a["w"], a["n_in"], a["gx"], None)
    for bad in (dict(gy=None), dict(pair=None), dict(offsets=None), dict(w=None), dict(gx=None), dict(c=0), dict(m=-1), dict(n_in=-1),
                dict(n_pair=-1), dict(n_pair=8 * n + 1), dict(m=ops.FIELD_MAX_POINTS + 1)):
        refused("osn_interp_bwd", ibwd(**bad))

    def sred(**kw):
        a = dict(x=a0, n=n, c=c, order=a1, offsets=a2, n_seg=4, mode=0, y=a3)
        a.update(kw)
        return h.osn_segment_reduce(a["x"], a["n"], a["c"], a["order"], a["offsets"], a["n_seg"], a["mode"], a["y"], None)
    for bad in (dict(x=None), dict(order=None), dict(offsets=None), dict(y=None), dict(c=0), dict(mode=2), dict(mode=-1), dict(n=-1),
                dict(n_seg=-1)):
        refused("osn_segment_reduce", sred(**bad))
    # sizes that need no launch are accepted without touching a pointer
    assert fmap(m=0, keys=None, pos=None, nbr=None) == 0 and ifwd(m=0, x=None, nbr=None, y=None) == 0
    assert ibwd(n_in=0, gy=None, offsets=None, gx=None) == 0 and sred(n_seg=0, x=None, offsets=None, y=None) == 0
