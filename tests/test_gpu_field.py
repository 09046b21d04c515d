"""TensorField, slice and trilinear interpolation on the GPU against tests/field_reference.py.

Every operation of csrc/field.hip is a pure function with a stated order: the corner table, the weights and
the invalid count, interpolation forward and backward, the three quantisation modes forward and backward and the slice forward
and backward are bit for bit the float32 numpy restatement, and two calls give the same bits.  Against the float64 form evaluated
from the same float32 t:  |y - y64| <= 12 * 2^-24 * sum_k w_k |x_k|  (first order: three roundings in a weight, one in the product,
seven in the sum, one of slack for the second order), and the same for gx with the list length + 4 in the place of 11 + 1.  The
network test uses the project's network tolerance (tests/test_gpu_unet.py: relative L2 <= 2e-4)."""
import functools

import numpy as np
import pytest
import torch

import field_reference as fr
from conv_bounds import adversarial

pytestmark = pytest.mark.gpu

F32 = np.float32
EPS = 2.0 ** -24
STRIDES = (1, 2, 4)
MODES = (("sum", "UNWEIGHTED_SUM"), ("avg", "UNWEIGHTED_AVERAGE"), ("first", "RANDOM_SUBSAMPLE"))
ALIAS_X = -25536                    # the cell pack_key would wrap x = 40000 onto: (40000 + 32768) mod 65536 - 32768


def dev():
    return torch.device("cuda", 0)


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def bits(a):
    """The bit patterns of a float32 array (every NaN as one pattern: which NaN 0 * inf makes is the machine's choice)."""
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    if a.dtype != np.float32:
        return a
    return np.where(np.isnan(a), np.int32(0x7FC00000), np.ascontiguousarray(a).view(np.int32))


def same_bits(got, want, what):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, "%s: shape %s against %s" % (what, g.shape, w.shape)
    bad = np.argwhere(g != w)
    assert bad.shape[0] == 0, "%s: %d elements differ, first at %s" % (what, bad.shape[0], bad[0])


def features(kind, n, c, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, c, generator=g) if kind == "randn" else adversarial("row_scales", n, c, g)).numpy().astype(F32)


# ---- the scene: a random cloud in two batches and the planted rows -----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene():
    """positions float32 [N, 4] of the field, and queries float32 [M, 4] = the field's points and the planted query rows."""
    rng = np.random.default_rng(0)
    xyz = rng.uniform(-3.0, 5.0, (150, 3))
    rows = [np.concatenate([np.full((150, 1), b), xyz], 1) for b in (0, 1)]          # two batches, identical spatial coordinates
    block = np.array([[x, y, z] for x in (8, 9, 10, 12) for y in (8, 9, 10, 12) for z in (8, 9, 10, 12)], np.float64) + 0.5
    rows.append(np.concatenate([np.zeros((64, 1)), block], 1))                       # every corner of base 8 at strides 1, 2, 4
    rows.append(np.array([[0, 40.5, 40.5, 40.5], [0, -0.25, 0.5, 0.5], [1, -0.25, -0.25, -0.25],       # a lone voxel; -0.25 -> cell -1
                          [0, ALIAS_X + 0.5, 0.5, 0.5]]))                            # the voxel a wrapped key of x = 40000.3 would hit
    rows.append(np.concatenate([np.zeros((600, 1)), 20 + rng.random((600, 3))], 1))  # one voxel of 600 points,
    rows.append(np.array([[0, 22.25, 20.5, 20.5], [0, 22.75, 20.5, 20.5]]))          # one of two (the lone voxel has one)
    pos = np.concatenate(rows).astype(F32)
    pos = pos[rng.permutation(pos.shape[0])]
    planted = np.array([[0, 8.3, 8.6, 8.1],               # -9: all eight corners, at every stride
                        [0, 40.25, 40.5, 40.75],          # -8: one corner
                        [0, 100.5, 100.5, 100.5],         # -7: none
                        [0, 8.0, 8.5, 8.5],               # -6: on a cell wall: the corners at x = 9 have weight 0
                        [0, np.nan, 0, 0],                # -5 .. -1: invalid rows
                        [0, 1, np.inf, 0], [-1, 0.5, 0.5, 0.5], [65535, 0.5, 0.5, 0.5],
                        [0, 40000.3, 0.5, 0.5]], np.float64).astype(F32)
    return pos, np.concatenate([pos, planted])


@functools.lru_cache(maxsize=None)
def built():
    """The field on the device with its manager, and the reference's quantisation of the same positions."""
    from openscene_amd.field import TensorField
    pos, _ = scene()
    field = TensorField(up(features("randn", pos.shape[0], 3, 1)), up(pos))
    x = field.sparse()
    uniq, inv, first, cnt = fr.quantize_map(pos)
    assert np.array_equal(x.C.cpu().numpy(), uniq) and sorted(set(cnt.tolist()) & {1, 2, 600}) == [1, 2, 600]
    same_bits(field.inverse_mapping, inv, "inverse_mapping")
    return field, uniq, inv, first, cnt


@functools.lru_cache(maxsize=None)
def level(s):
    """(coords of the stride's map in the product's row order, reference corner table / weights / invalid / t / valid of the queries)."""
    field = built()[0]
    coords_s = field.coordinate_manager.coords(s).cpu().numpy()
    return (coords_s,) + fr.interp_map(coords_s, scene()[1], s)


def tensor_at(s, c, kind="randn", seed=2):
    from openscene_amd.sparse import SparseTensor
    cm = built()[0].coordinate_manager
    x = features(kind, cm.size(s), c, seed + s)
    return x, SparseTensor(up(x).requires_grad_(True), tensor_stride=s, coordinate_manager=cm)


# ---- 1. the map ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", STRIDES)
def test_map_is_the_restatement_bit_for_bit(s):
    from openscene_amd.field import InterpolationMap
    cm = built()[0].coordinate_manager
    coords_s, nbr, w, bad, t, valid = level(s)
    q = up(scene()[1])
    a, b = InterpolationMap(cm, s, q), InterpolationMap(cm, s, q)
    same_bits(a.nbr, nbr, "nbr")
    same_bits(a.w, w, "w")
    same_bits(b.nbr, a.nbr, "nbr, second call")
    same_bits(b.w, a.w, "w, second call")
    assert a.invalid == bad == 5 and b.invalid == 5
    # the planted rows are what they were planted for
    present = (nbr >= 0).sum(0)
    assert present[-9] == 8 and present[-8] == 1 and present[-7] == 0 and valid[-7] and present[-6] == 8
    assert not valid[-5:].any() and (nbr[:, -5:] == -1).all() and not w[:, -5:].any()
    assert (coords_s[:, 1] == ALIAS_X).any() and ALIAS_X % 4 == 0                   # the aliased voxel exists at this stride
    neg = np.nonzero((scene()[1][:, 1] == F32(-0.25)) & (scene()[1][:, 0] == 0))[0][0]
    assert coords_s[nbr[0, neg]].tolist()[1] == -s                                   # floor, not truncation: base -1 / -2 / -4


@pytest.mark.parametrize("s", STRIDES)
def test_lattice_sites_return_the_voxel_rows(s):
    x, sp = tensor_at(s, 5)
    y = sp.features_at_coordinates(sp.C.float())
    same_bits(y, x, "rows at their own lattice sites")


# ---- 2. interpolation ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [3, 32])
@pytest.mark.parametrize("s", STRIDES)
def test_interpolation_forward_and_backward_bit_for_bit(s, c):
    coords_s, nbr, w, bad, t, valid = level(s)
    x, sp = tensor_at(s, c)
    q = scene()[1]
    if s == 1:                                    # an inf in a voxel whose weight is 0 for the point on the cell wall: 0 * inf = NaN
        x = x.copy()
        x[nbr[1, -6]] = np.inf
        assert w[1, -6] == 0 and nbr[1, -6] >= 0
        sp = sp._like(up(x).requires_grad_(True))
    y = sp.features_at_coordinates(up(q))
    want = fr.interp_fwd(x, nbr, w)
    same_bits(y, want, "y")
    if s == 1:
        assert np.isnan(want[-6]).all() and torch.isnan(y[-6]).all()
    assert not want[-7].any() and not np.signbit(want[-7]).any()                    # no corner: a row of +0
    gy = features("randn", q.shape[0], c, 3)
    (gx,) = torch.autograd.grad(y, sp.F, up(gy))
    same_bits(gx, fr.interp_bwd(gy, nbr, w, coords_s.shape[0]), "gx")
    y2 = sp.features_at_coordinates(up(q))
    (gx2,) = torch.autograd.grad(y2, sp.F, up(gy))
    same_bits(y2, y, "y, second call")
    same_bits(gx2, gx, "gx, second call")


def test_a_voxel_no_point_touches_gets_a_written_zero():
    from openscene_amd import ops
    from openscene_amd.field import InterpolationMap
    cm = built()[0].coordinate_manager
    q = scene()[1][-9:]                                                            # the planted rows alone: most voxels have no pair
    imap = InterpolationMap(cm, 1, up(q))
    gy = features("randn", 9, 4, 4)
    out = torch.full((cm.size(1), 4), float("nan"), device=dev())
    gx = ops.interp_bwd(up(gy), imap.plan(), imap.w, cm.size(1), out=out)
    assert gx is out
    want = fr.interp_bwd(gy, imap.nbr.cpu().numpy(), imap.w.cpu().numpy(), cm.size(1))
    same_bits(gx, want, "gx over a NaN-filled destination")
    assert (~want.any(1)).sum() > cm.size(1) - 20 and not np.signbit(want[~want.any(1)]).any()


@pytest.mark.parametrize("kind", ["randn", "row_scales"])
def test_interpolation_within_the_float64_bound(kind):
    for s in STRIDES:
        coords_s, nbr, w, bad, t, valid = level(s)
        x, sp = tensor_at(s, 8, kind, seed=5)
        q = scene()[1]
        y = sp.features_at_coordinates(up(q))
        w64 = fr.weights64(t, valid)
        y64, a64 = fr.interp_fwd64(x, nbr, w64)
        err = np.abs(y.detach().cpu().numpy().astype(np.float64) - y64)
        print("stride %d %s: forward worst err / (2^-24 abs-sum) = %.2f" % (s, kind, float((err / np.maximum(EPS * a64, 1e-300)).max())))
        assert (err <= 12 * EPS * a64).all()
        gy = features(kind, q.shape[0], 8, 6)
        (gx,) = torch.autograd.grad(y, sp.F, up(gy))
        gx64, b64, length = fr.interp_bwd64(gy, nbr, w64, coords_s.shape[0])
        gerr = np.abs(gx.cpu().numpy().astype(np.float64) - gx64)
        print("stride %d %s: backward worst err / ((len + 4) 2^-24 abs-sum) = %.2f"
              % (s, kind, float((gerr / np.maximum((length[:, None] + 4) * EPS * b64, 1e-300)).max())))
        assert (gerr <= (length[:, None] + 4) * EPS * b64).all()


# ---- 3. quantisation ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [3, 32])
@pytest.mark.parametrize("word,name", MODES)
def test_quantisation_forward_and_backward_bit_for_bit(word, name, c):
    from openscene_amd.field import SparseTensorQuantizationMode, TensorField
    from openscene_amd.sparse import SparseTensor
    _, uniq, inv, first, cnt = built()
    pos = scene()[0]
    x = features("row_scales", pos.shape[0], c, 7)
    gy = features("randn", uniq.shape[0], c, 8)
    mode = SparseTensorQuantizationMode[name]
    outs = []
    for _ in range(2):
        f = up(x).requires_grad_(True)
        sp = TensorField(f, up(pos), quantization_mode=mode).sparse()
        (gx,) = torch.autograd.grad(sp.F, f, up(gy))
        outs.append((sp.F.detach(), gx))
    same_bits(outs[0][0], fr.quantize_fwd(x, inv, first, cnt, word), "voxel rows")
    same_bits(outs[0][1], fr.quantize_bwd(gy, inv, first, cnt, word), "point gradients")
    same_bits(outs[1][0], outs[0][0], "voxel rows, second call")
    same_bits(outs[1][1], outs[0][1], "point gradients, second call")
    # duplicate INTEGER coordinates of a SparseTensor take the same three modes; the default stays the first row
    ci = up(fr.cells(pos))
    same_bits(SparseTensor(up(x), ci, quantization_mode=mode).F, outs[0][0], "SparseTensor(quantization_mode=)")
    same_bits(SparseTensor(up(x), ci).F, x[first], "SparseTensor default")


# ---- 4. slice ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", STRIDES)
def test_slice_forward_and_backward_bit_for_bit(s):
    from openscene_amd.field import TensorField
    field, uniq, inv, first, cnt = built()
    coords_s = level(s)[0]
    where = {tuple(r): i for i, r in enumerate(coords_s.tolist())}
    cells = fr.cells(scene()[0]).astype(np.int64)
    cells[:, 1:] = np.floor_divide(cells[:, 1:], s) * s
    inv_s = np.array([where[tuple(r)] for r in cells.tolist()], np.int64)          # from the coordinates alone
    x, sp = tensor_at(s, 6)
    out = sp.slice(field)
    assert out.C is field.C
    same_bits(out.F, x[inv_s], "slice")
    if s == 1:
        same_bits(out.F, sp.F[field.inverse_mapping], "slice against F[inverse_mapping]")
    gy = features("row_scales", inv_s.shape[0], 6, 9)
    (gx,) = torch.autograd.grad(out.F, sp.F, up(gy))
    same_bits(gx, fr.ordered_sum(gy, inv_s, coords_s.shape[0]), "slice backward")
    (gx2,) = torch.autograd.grad(sp.slice(field).F, sp.F, up(gy))
    same_bits(gx2, gx, "slice backward, second call")
    same_bits(sp.cat_slice(field).F, np.concatenate([x[inv_s], field.F.detach().cpu().numpy()], 1), "cat_slice")
    other = TensorField(field.F.detach(), field.C)
    other.sparse()
    with pytest.raises(ValueError):
        sp.slice(other)


# ---- 5. shapes: 0, 1, around a wave, more than one block; the vector path, the scalar path, a misaligned base ----------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_shapes(n):
    from openscene_amd import ops
    field, uniq, inv, first, cnt = built()
    cm = field.coordinate_manager
    coords1, nbr_all, w_all = level(1)[:3]
    q = scene()[1][-n:] if n else scene()[1][:0]                                     # the planted rows are among them from n = 63 on
    nbr, w = np.ascontiguousarray(nbr_all[:, nbr_all.shape[1] - n:]), np.ascontiguousarray(w_all[:, w_all.shape[1] - n:])
    got_nbr, got_w, bad = ops.field_map(cm._tables[1], up(q), 1)
    same_bits(got_nbr, nbr, "nbr"), same_bits(got_w, w, "w")
    assert int(bad) == (5 if n >= 5 else n)
    plan = ops.interp_plan(got_nbr, cm.size(1))
    # N = n points in n_seg voxels: the first n points of the scene, re-ranked
    seg = inv[:n]
    ids, seg = np.unique(seg, return_inverse=True) if n else (np.zeros(0, np.int64), np.zeros(0, np.int64))
    order, offsets, _ = fr.csr(seg, ids.shape[0])
    for c in (1, 3, 4, 32, 96):
        for misaligned in ((False, True) if c % 4 == 0 else (False,)):
            def put(a):
                if not misaligned or a.size == 0:
                    return up(a)
                buf = torch.empty(a.size + 1, dtype=torch.float32, device=dev())
                v = buf[1:].view(a.shape)
                v.copy_(torch.from_numpy(a))
                assert v.data_ptr() % 16 == 4 and v.is_contiguous()
                return v
            x = features("randn", coords1.shape[0], c, 10 + c)
            same_bits(ops.interp_fwd(put(x), got_nbr, got_w), fr.interp_fwd(x, nbr, w), "interp_fwd c=%d" % c)
            gy = features("randn", n, c, 20 + c)
            same_bits(ops.interp_bwd(put(gy), plan, got_w, cm.size(1)), fr.interp_bwd(gy, nbr, w, coords1.shape[0]), "interp_bwd c=%d" % c)
            xs = features("row_scales", n, c, 30 + c)
            for mode in ("sum", "avg"):
                want = fr.ordered_sum(xs, seg, ids.shape[0])
                if mode == "avg":
                    want = want / np.diff(offsets).astype(F32)[:, None]
                same_bits(ops.segment_reduce(put(xs), up(order.astype(np.int32)), up(offsets), mode), want, "segment_reduce %s c=%d" % (mode, c))
                g = features("randn", ids.shape[0], c, 40 + c)
                want = g[seg] / np.diff(offsets).astype(F32)[seg][:, None] if mode == "avg" else g[seg]
                same_bits(ops.segment_expand(put(g), up(seg.astype(np.int32)), up(offsets), mode), want, "segment_expand %s c=%d" % (mode, c))


# ---- 6. end to end -----------------------------------------------------------------------------------------------------------------
def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm())


def test_field_to_points_through_a_small_network():
    from openscene_amd import minkowski as mk
    rng = np.random.default_rng(11)
    xyz = rng.uniform(0.0, 9.0, (1000, 3))
    pos = np.concatenate([np.concatenate([np.full((1000, 1), b), xyz + 0.37 * b], 1) for b in (0, 1)]).astype(F32)
    feats = features("randn", 2000, 3, 12)
    torch.manual_seed(0)
    conv1 = mk.MinkowskiConvolution(3, 16, kernel_size=3, dimension=3).to(dev())
    conv2 = mk.MinkowskiConvolution(16, 16, kernel_size=2, stride=2, dimension=3).to(dev())
    f = up(feats).requires_grad_(True)
    field = mk.TensorField(f, up(pos))
    out = conv2(conv1(field.sparse()))
    y = out.interpolate(field)
    y.F.square().sum().backward()
    f64 = torch.from_numpy(feats).double().requires_grad_(True)
    w1, w2 = conv1.kernel.detach().double().cpu().requires_grad_(True), conv2.kernel.detach().double().cpu().requires_grad_(True)
    y64, _, _ = fr.chain64(f64, pos, w1, w2)
    y64.square().sum().backward()
    errs = dict(y=rel(y.F, y64), gf=rel(f.grad, f64.grad), gw1=rel(conv1.kernel.grad, w1.grad), gw2=rel(conv2.kernel.grad, w2.grad))
    print("relative L2 against float64:", {k: "%.2e" % v for k, v in errs.items()})
    assert all(v <= 2e-4 for v in errs.values()), errs
    h = conv1(field.sparse())
    same_bits(h.slice(field).F, h.F[field.inverse_mapping], "out.slice(field).F against out.F[field.inverse_mapping]")
    same_bits(out.slice(field).F, out.F[field.coordinate_manager.point_index(2).rank.long()], "the same at stride 2")
