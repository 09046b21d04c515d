"""Sparse pooling layers on the GPU against tests/pooling_reference.py.

Local pooling (forward y / arg / cnt, backward gx) and the backward of the global and broadcast layers are pure functions with a
stated order: bit for bit the float32 numpy restatement.  Global sums are held to the first-order bound of a chunked sum, any fixed
order inside a chunk of G = ops.GPOOL_CHUNK rows, then p ordered adds: |err| <= (G + p + 1) * 2^-24 * sum |x|; on integer-valued
rows every partial sum is exact and the result is bit for bit the int64 sum.  The network test uses the project's network tolerance
(tests/test_gpu_unet.py: relative L2 <= 2e-4 on the fp32 run's ReLU activation pattern)."""
import functools

import numpy as np
import pytest
import torch

import pooling_reference as pr
from conv_bounds import adversarial
from oracle import coords as oc
from openscene_amd import synthetic as syn

pytestmark = pytest.mark.gpu

MODES = ("sum", "avg", "max")


def dev():
    return torch.device("cuda", 0)


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.int32) if a.dtype == np.float32 else a


def same_bits(got, want, what):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, "%s: shape %s against %s" % (what, g.shape, w.shape)
    bad = np.argwhere(g != w)
    assert bad.shape[0] == 0, "%s: %d elements differ, first at %s" % (what, bad.shape[0], bad[0])


def features(kind, n, c, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, c, generator=g) if kind == "randn" else adversarial("row_scales", n, c, g)).numpy()


# ---- 1. local pooling, bit for bit ------------------------------------------------------------------------------------------
def grid_coords(seed, side=12, p=0.22, batches=2):
    rng = np.random.default_rng(seed)
    rows = []
    for b in range(batches):
        occ = rng.random((side, side, side)) < p
        if b == 0:
            occ[3:6, 3:6, 3:6] = True             # a solid 3^3 block around the even cell (4, 4, 4): a row with every neighbour
        else:
            occ[9:12, 9:12, 9:12] = False         # ... and a lone voxel: a row with a single neighbour, on every map kind
            occ[10, 10, 10] = True
        g = np.argwhere(occ).astype(np.int32)
        rows.append(np.concatenate([np.full((g.shape[0], 1), b, np.int32), g], 1))
    c = np.concatenate(rows)
    return c[rng.permutation(c.shape[0])]


@functools.lru_cache(maxsize=None)
def local_map(name):
    """(n_in, nbr_fwd, nbr_bwd, flip): the three map kinds on a 12^3 grid with two batches, and hand-made tables of K = 8 with
    1 / 63 / 64 / 65 output rows (a row with every neighbour, one with a single neighbour, absent entries elsewhere)."""
    if name.startswith("hand"):
        n_out, n_in, K = int(name[4:]), 70, 8
        rng = np.random.default_rng(n_out)
        nbr = np.stack([rng.permutation(n_in)[:n_out] for _ in range(K)]).astype(np.int32)      # (an offset names an input once)
        absent = rng.random(nbr.shape) < 0.4
        absent[:, 0] = False
        if n_out > 1:
            absent[:, 1] = True
            absent[0, 1] = False
        nbr[absent] = -1
        return n_in, nbr, oc.transpose_table(nbr, n_in), False
    ksize, stride = {"k2s2": (2, 2), "k3s1": (3, 1), "k3s2": (3, 2)}[name]
    fine = grid_coords(5)
    out = fine if stride == 1 else oc.stride_map(fine, stride)[0]
    nbr, nbr_bwd, flip = pr.tables(fine, out, ksize)
    cnt = (nbr >= 0).sum(0)
    assert 500 <= fine.shape[0] <= 1000 and cnt.min() == 1 and cnt.max() == ksize ** 3, (fine.shape, cnt.min(), cnt.max())
    return fine.shape[0], nbr, nbr_bwd, flip


@pytest.mark.parametrize("kind", ["randn", "row_scales"])
@pytest.mark.parametrize("c", [1, 3, 32, 96, 100])
@pytest.mark.parametrize("name", ["k2s2", "k3s1", "k3s2", "hand1", "hand63", "hand64", "hand65"])
def test_local_pooling_bitwise(name, c, kind):
    from openscene_amd import ops
    n_in, nbr, nbr_bwd, flip = local_map(name)
    n_out = nbr.shape[1]
    x, gy = features(kind, n_in, c, 1), features(kind, n_out, c, 2)
    d_nbr, d_bwd = up(nbr), (up(nbr) if flip else up(nbr_bwd))
    d_cnt = ops.pool_count(d_nbr, n_in)
    for mode in MODES:
        y, arg, cnt = pr.local_fwd(x, nbr, mode)
        gx = pr.local_bwd(gy, nbr_bwd, flip, mode, cnt=cnt, arg=arg)
        got_y, got_arg = ops.pool_fwd(up(x), d_nbr, mode)
        same_bits(got_y, y, "%s y" % mode)
        same_bits(d_cnt, cnt, "cnt")
        if mode == "max":
            same_bits(got_arg, arg, "arg")
        else:
            assert got_arg is None
        got_gx = ops.pool_bwd(up(gy), d_bwd, flip, mode, cnt=d_cnt, arg=got_arg)
        same_bits(got_gx, gx, "%s gx" % mode)


@pytest.mark.parametrize("ksize,stride", [(2, 2), (3, 1), (3, 2)])
def test_local_pooling_modules_on_the_managers_maps(ksize, stride):
    """The modules on CoordinateManager.kmap's own tables (the mirror flag, the transposed table, the cached divisor) through
    autograd: the same bits as the restatement on the oracle's tables."""
    from openscene_amd import minkowski as me
    from openscene_amd.sparse import SparseTensor
    fine = grid_coords(9)
    out = fine if stride == 1 else oc.stride_map(fine, stride)[0]
    nbr, nbr_bwd, flip = pr.tables(fine, out, ksize)
    x, gy = features("randn", fine.shape[0], 12, 3), features("randn", out.shape[0], 12, 4)
    for mode, cls in zip(MODES, (me.MinkowskiSumPooling, me.MinkowskiAvgPooling, me.MinkowskiMaxPooling)):
        xin = up(x).requires_grad_(True)
        res = cls(ksize, stride, dimension=3)(SparseTensor(xin, up(fine)))
        assert res.tensor_stride == stride and np.array_equal(res.C.cpu().numpy(), out)
        res.F.backward(up(gy))
        y, arg, cnt = pr.local_fwd(x, nbr, mode)
        same_bits(res.F, y, "%s y" % mode)
        same_bits(xin.grad, pr.local_bwd(gy, nbr_bwd, flip, mode, cnt=cnt, arg=arg), "%s gx" % mode)


# ---- 2. max pooling rules --------------------------------------------------------------------------------------------------
def test_max_pooling_rules():
    from openscene_amd import ops
    col = np.array([3, 1, 4, -1, 0, 2, -1, 5], np.int32)          # output row 0: input rows by k
    nbr = np.stack([col, np.array([-1, 6, -1, 7, -1, 3, -1, -1], np.int32)], 1)      # (a second output row that shares input row 3)
    rng = np.random.default_rng(0)
    x = rng.standard_normal((8, 8)).astype(np.float32) - 10
    x[[1, 0], 0] = 2.5                                             # equal maxima at k = 1 (row 1) and k = 4 (row 0)
    x[:, 1] = -1; x[3, 1] = 0.0; x[1, 1] = -0.0                    # +0 at k = 0, -0 at k = 1
    x[:, 2] = -1; x[3, 2] = -0.0; x[1, 2] = 0.0                    # -0 at k = 0, +0 at k = 1
    x[4, 3] = np.nan; x[2, 3] = np.nan; x[3, 3] = 1e30             # NaNs at k = 2 (row 4) and k = 5 (row 2)
    x[:, 4] = -np.inf                                              # nothing but -inf
    y, arg = ops.pool_fwd(up(x), up(nbr), "max")
    ry, rarg, _ = pr.local_fwd(x, nbr, "max")
    same_bits(y, ry, "y")
    same_bits(arg, rarg, "arg")
    y, arg = y.cpu().numpy(), arg.cpu().numpy()
    assert arg[0, 0] == 1 and y[0, 0] == 2.5
    assert arg[0, 1] == 3 and y[0, 1] == 0 and not np.signbit(y[0, 1])
    assert arg[0, 2] == 3 and y[0, 2] == 0 and np.signbit(y[0, 2])
    assert arg[0, 3] == 4 and np.isnan(y[0, 3])
    assert arg[0, 4] == 3 and y[0, 4] == -np.inf
    # the gradient lands on exactly the arg row
    gy = np.full((2, 8), 7.0, np.float32)
    gy[1] = 11.0
    gx = ops.pool_bwd(up(gy), up(oc.transpose_table(nbr, 8)), False, "max", arg=up(rarg)).cpu().numpy()
    want = np.zeros((8, 8), np.float32)
    for o in range(2):
        for c in range(8):
            want[rarg[o, c], c] += gy[o, c]
    same_bits(gx, want, "gx")
    assert gx[1, 0] == 7.0 and gx[0, 0] == 0.0 and gx[4, 3] == 7.0 and gx[2, 3] == 0.0
    same_bits(gx, pr.local_bwd(gy, oc.transpose_table(nbr, 8), False, "max", arg=rarg), "gx against the restatement")


# ---- 3-6. global pooling and broadcast -----------------------------------------------------------------------------------------
class Layout:
    """Batches of 1, G - 1, G, G + 1 and 3 G - 7 rows under the ids 0, 2, 5, 6, 9, rows interleaved by a seeded permutation."""

    def __init__(self):
        from openscene_amd import ops
        from openscene_amd.sparse import CoordinateManager
        self.G = G = ops.GPOOL_CHUNK
        assert G <= 512
        self.sizes, self.ids = [1, G - 1, G, G + 1, 3 * G - 7], [0, 2, 5, 6, 9]
        b = np.concatenate([np.full(m, i, np.int32) for m, i in zip(self.sizes, self.ids)])
        self.b = b[np.random.default_rng(7).permutation(b.shape[0])]
        self.n = self.b.shape[0]
        coords = np.zeros((self.n, 4), np.int32)
        coords[:, 0], coords[:, 1] = self.b, np.arange(self.n)
        self.cm = CoordinateManager(up(coords))
        self.index = self.cm.batch_index(1)


@pytest.fixture(scope="module")
def layout():
    return Layout()


def test_batch_index_of_the_layout(layout):
    idx = layout.index
    ids, rank, counts = pr.batch_index(layout.b)
    assert idx.ids.tolist() == layout.ids == ids.tolist() and counts.tolist() == layout.sizes
    assert np.array_equal(idx.rank.cpu().numpy(), rank) and idx.offsets.tolist() == [0] + np.cumsum(counts).tolist()
    order = idx.order.cpu().numpy()
    for j in range(5):
        assert np.array_equal(order[idx.offsets[j]:idx.offsets[j + 1]], np.nonzero(rank == j)[0])
    assert (idx.ids.dtype, idx.rank.dtype, idx.order.dtype, idx.offsets.dtype) == (torch.int32,) * 3 + (torch.int64,)
    assert layout.cm.batch_index(1) is idx and any(t is idx.order for t in layout.cm.tensors())
    layout.cm.record_stream(torch.cuda.current_stream(dev()))


@pytest.mark.parametrize("c", [1, 32, 100])
def test_global_sums_lose_no_row(layout, c):
    from openscene_amd import ops
    x = np.random.default_rng(c).integers(-8, 9, (layout.n, c)).astype(np.float32)
    ids, rank, counts = pr.batch_index(layout.b)
    exact = np.zeros((5, c), np.int64)
    np.add.at(exact, rank, x.astype(np.int64))
    y, arg = ops.gpool_fwd(up(x), layout.index.order, layout.index.offsets, "sum")
    assert arg is None
    same_bits(y, exact.astype(np.float32), "sum")
    y, _ = ops.gpool_fwd(up(x), layout.index.order, layout.index.offsets, "avg")
    same_bits(y, exact.astype(np.float32) / counts.astype(np.float32)[:, None], "avg")


@pytest.mark.parametrize("kind", ["randn", "row_scales"])
@pytest.mark.parametrize("c", [1, 32, 100])
def test_global_pooling_float_inputs(layout, c, kind):
    from openscene_amd import ops
    x = features(kind, layout.n, c, 10 + c)
    ids, rank, counts = pr.batch_index(layout.b)
    mag = np.zeros((5, c))
    np.add.at(mag, rank, np.abs(x.astype(np.float64)))
    bound = pr.sum_bound(mag, counts, layout.G)
    want, _, _ = pr.global_fwd64(x, layout.b, "sum")
    y, _ = ops.gpool_fwd(up(x), layout.index.order, layout.index.offsets, "sum")
    err = np.abs(y.cpu().numpy().astype(np.float64) - want)
    print("sum: worst err / bound %.3f" % float((err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all()
    want = want / counts[:, None]
    y, _ = ops.gpool_fwd(up(x), layout.index.order, layout.index.offsets, "avg")
    err = np.abs(y.cpu().numpy().astype(np.float64) - want)
    lim = bound / counts[:, None] + 2.0 ** -24 * np.abs(want)
    print("avg: worst err / bound %.3f" % float((err / np.maximum(lim, 1e-300)).max()))
    assert (err <= lim).all()
    # max: exact; planted ties (two, and three with a +0 / -0 pair) go to the lowest row
    rows4 = np.nonzero(rank == 4)[0]
    x[rows4[[900, 17, 1400]], 0] = 1e9
    if c > 1:
        x[rows4, c - 1] = -np.abs(x[rows4, c - 1]) - 1
        x[rows4[[1000, 40]], c - 1] = [0.0, -0.0]
    want, warg, _ = pr.global_fwd64(x, layout.b, "max")
    y, arg = ops.gpool_fwd(up(x), layout.index.order, layout.index.offsets, "max")
    same_bits(y, want.astype(np.float32), "max")
    same_bits(arg, warg, "arg")
    arg = arg.cpu().numpy()
    assert arg[4, 0] == rows4[17]
    if c > 1:
        assert arg[4, c - 1] == rows4[40] and np.signbit(y.cpu().numpy()[4, c - 1])      # the value of the lowest row: -0
    # NaN propagates, arg at the lowest NaN row
    x[rows4[[1200, 300]], 0] = np.nan
    y, arg = ops.gpool_fwd(up(x), layout.index.order, layout.index.offsets, "max")
    assert np.isnan(y.cpu().numpy()[4, 0]) and arg.cpu().numpy()[4, 0] == rows4[300]
    assert not np.isnan(y.cpu().numpy()[:4]).any()


@pytest.mark.parametrize("c", [3, 32])
def test_placement_independence_and_repeatability(layout, c):
    """A batch's bits depend on its own rows only: alone, or interleaved with four other batches under another id."""
    from openscene_amd import ops
    from openscene_amd.sparse import CoordinateManager
    x = features("row_scales", layout.n, c, 20)
    ids, rank, counts = pr.batch_index(layout.b)
    rows = np.nonzero(rank == 4)[0]                                   # id 9, 3 G - 7 rows, scattered
    alone = np.zeros((rows.shape[0], 4), np.int32)
    alone[:, 1] = np.arange(rows.shape[0])
    one = CoordinateManager(up(alone)).batch_index(1)
    assert one.ids.tolist() == [0]
    gy = features("randn", 5, c, 21)
    for mode in MODES:
        a, a_arg = ops.gpool_fwd(up(x[rows]), one.order, one.offsets, mode)
        m, m_arg = ops.gpool_fwd(up(x), layout.index.order, layout.index.offsets, mode)
        same_bits(a[0], m[4], mode)
        if mode == "max":
            assert np.array_equal(rows[a_arg.cpu().numpy()[0]], m_arg.cpu().numpy()[4])
        m2, m2_arg = ops.gpool_fwd(up(x), layout.index.order, layout.index.offsets, mode)
        same_bits(m2, m, mode + " twice")
        g1 = ops.gpool_bwd(up(gy), layout.index.rank, layout.index.offsets, layout.n, mode, arg=m_arg)
        g2 = ops.gpool_bwd(up(gy), layout.index.rank, layout.index.offsets, layout.n, mode, arg=m2_arg)
        same_bits(g1, g2, mode + " backward twice")
    pooled, gout = features("randn", 5, c, 22), features("randn", layout.n, c, 23)
    for op in ("add", "mul"):
        r = [(ops.broadcast_fwd(up(x), up(pooled), layout.index.rank, op),
              ops.broadcast_bwd_pooled(up(gout), up(x) if op == "mul" else None, layout.index.order, layout.index.offsets))
             for _ in range(2)]
        same_bits(r[0][0], r[1][0], op + " twice")
        same_bits(r[0][1], r[1][1], op + " pooled gradient twice")
        alone_gg = ops.broadcast_bwd_pooled(up(gout[rows]), up(x[rows]) if op == "mul" else None, one.order, one.offsets)
        same_bits(alone_gg[0], r[0][1][4], op + " pooled gradient alone")


@pytest.mark.parametrize("c", [1, 32, 100])
def test_backward_of_global_and_broadcast(layout, c):
    from openscene_amd import functional as F_, ops
    idx = layout.index
    x, gy = features("row_scales", layout.n, c, 30), features("randn", 5, c, 31)
    for mode in MODES:
        xin = up(x).requires_grad_(True)
        y = F_.global_pool(xin, idx, mode)
        y.backward(up(gy))
        arg = pr.global_fwd64(x, layout.b, mode)[1]
        same_bits(xin.grad, pr.global_bwd(gy, layout.b, mode, arg=arg), mode + " gx")
    pooled, gout = features("randn", 5, c, 32), features("randn", layout.n, c, 33)
    for op in ("add", "mul"):
        xin, gin = up(x).requires_grad_(True), up(pooled).requires_grad_(True)
        y = F_.broadcast(xin, gin, idx, op)
        same_bits(y, pr.broadcast_fwd(x, pooled, layout.b, op), op + " y")
        y.backward(up(gout))
        gx, gg, mag = pr.broadcast_bwd64(gout, x, pooled, layout.b, op)
        same_bits(xin.grad, gx, op + " gx")
        err = np.abs(gin.grad.cpu().numpy().astype(np.float64) - gg)
        bound = pr.sum_bound(mag, np.array(layout.sizes), layout.G)
        print("%s gg: worst err / bound %.3f" % (op, float((err / np.maximum(bound, 1e-300)).max())))
        assert (err <= bound).all()
        # integer-valued operands: every partial sum is exact
        xi = np.random.default_rng(34).integers(-8, 9, (layout.n, c)).astype(np.float32)
        gi = np.random.default_rng(35).integers(-8, 9, (layout.n, c)).astype(np.float32)
        got = ops.broadcast_bwd_pooled(up(gi), up(xi) if op == "mul" else None, idx.order, idx.offsets)
        same_bits(got, pr.broadcast_bwd64(gi, xi, pooled, layout.b, op)[1].astype(np.float32), op + " gg on integers")


# ---- 7. edges ------------------------------------------------------------------------------------------------------------------
def test_empty_tensor_through_every_layer():
    from openscene_amd import minkowski as me
    from openscene_amd.sparse import ORIGIN_STRIDE, SparseTensor
    x = SparseTensor(torch.zeros(0, 8, device=dev(), requires_grad=True), torch.zeros(0, 4, dtype=torch.int32, device=dev()))
    for cls in (me.MinkowskiSumPooling, me.MinkowskiAvgPooling, me.MinkowskiMaxPooling):
        for k, s in ((2, 2), (3, 1), (3, 2)):
            y = cls(k, s)(x)
            assert y.F.shape == (0, 8) and y.tensor_stride == s
    for cls in (me.MinkowskiGlobalSumPooling, me.MinkowskiGlobalAvgPooling, me.MinkowskiGlobalMaxPooling):
        g = cls()(x)
        assert g.F.shape == (0, 8) and g.tensor_stride == ORIGIN_STRIDE and g.C.shape == (0, 4)
        for b in (me.MinkowskiBroadcastAddition(), me.MinkowskiBroadcastMultiplication()):
            assert b(x, g).F.shape == (0, 8)
        out = me.MinkowskiLinear(8, 4).to(dev())(g)
        assert out.F.shape == (0, 4)
        (out.F.sum() + me.MinkowskiBroadcastMultiplication()(x, g).F.sum()).backward()
    torch.cuda.synchronize()


def test_pooled_tensor_is_refused_by_spatial_layers_and_maps_are_shared():
    from openscene_amd import minkowski as me
    from openscene_amd.sparse import ORIGIN_STRIDE, SparseTensor
    fine = grid_coords(11)
    x = SparseTensor(up(features("randn", fine.shape[0], 8, 40)), up(fine))
    cm = x.coordinate_manager
    pooled = me.MinkowskiGlobalAvgPooling()(x)
    assert pooled.tensor_stride == ORIGIN_STRIDE and pooled.coordinate_manager is cm
    assert pooled.C.tolist() == [[0, 0, 0, 0], [1, 0, 0, 0]] and pooled.C.dtype == torch.int32 and pooled.F.shape == (2, 8)
    # feature-only layers take it
    assert me.MinkowskiReLU()(pooled).F.shape == (2, 8) and (pooled + pooled).F.shape == (2, 8) and me.cat(pooled, pooled).F.shape == (2, 16)
    assert me.MinkowskiBatchNorm(8).to(dev())(pooled).F.shape == (2, 8) and me.MinkowskiLinear(8, 5).to(dev())(pooled).F.shape == (2, 5)
    for layer in (me.MinkowskiConvolution(8, 8, kernel_size=3, dimension=3).to(dev()), me.MinkowskiAvgPooling(2, 2), me.MinkowskiMaxPooling(3)):
        with pytest.raises(ValueError, match="globally pooled"):
            layer(pooled)
    with pytest.raises(ValueError):
        me.MinkowskiBroadcastAddition()(x, x)
    # a local pooling and a convolution of the same geometry share one cached map
    for k, s in ((2, 2), (3, 1)):
        me.MinkowskiConvolution(8, 8, kernel_size=k, stride=s, dimension=3).to(dev())(x)
        before = set(cm._kmaps)
        me.MinkowskiMaxPooling(k, s)(x)
        me.MinkowskiSumPooling(k, s)(x)
        assert set(cm._kmaps) == before
        me.MinkowskiAvgPooling(k, s)(x)
        assert set(cm._kmaps) - before == {("pool_cnt", 1, s, k, 1)}             # only the average's divisor, next to its map


# ---- 8. a network end to end --------------------------------------------------------------------------------------------------
def rel_l2(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return ((got - ref).norm() / (ref.norm() + 1e-30)).item()


def build_net(kind):
    from openscene_amd import minkowski as me

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.conv = me.MinkowskiConvolution(3, 32, kernel_size=3, dimension=3)
            self.bn = me.MinkowskiBatchNorm(32)
            self.relu = me.MinkowskiReLU()
            self.pool = (me.MinkowskiAvgPooling if kind == "avg" else me.MinkowskiMaxPooling)(2, 2)
            self.block = me.BasicBlock(32, 64, downsample=torch.nn.Sequential(
                me.MinkowskiConvolution(32, 64, kernel_size=1, dimension=3), me.MinkowskiBatchNorm(64)), dimension=3)
            self.gpool = me.MinkowskiGlobalAvgPooling() if kind == "avg" else me.MinkowskiGlobalMaxPooling()
            self.se = me.MinkowskiLinear(64, 64)
            self.gate = me.MinkowskiBroadcastMultiplication()
            self.final = me.MinkowskiLinear(64, 4)

        def forward(self, x):
            x = self.block(self.pool(self.relu(self.bn(self.conv(x)))))
            x = self.gate(x, self.se(self.gpool(x)))
            return self.final(self.gpool(x)).F

    torch.manual_seed(3)
    net = Net()
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm1d):
            m.weight.data.uniform_(0.5, 1.5)
            m.bias.data.uniform_(-0.3, 0.3)
    return net.train()


def scenes():
    coords = syn.batch_coords([syn.shuffled(syn.grid_voxels(syn.room_points(31 + b, n_pts=2100), 0.05), 31 + b) for b in range(2)])
    return coords, torch.rand(coords.shape[0], 3, generator=torch.Generator().manual_seed(5))


def test_network_with_average_pooling_against_float64():
    from openscene_amd import functional as F_
    from openscene_amd.sparse import SparseTensor
    net = build_net("avg")
    coords, feats = scenes()
    labels = torch.tensor([1, 3])
    p = {k: v.detach().clone().double() for k, v in net.state_dict().items() if v.dtype.is_floating_point}
    for k, v in p.items():
        if "running" not in k:
            v.requires_grad_(True)
    free = pr.pooled_net_forward({k: v.detach().clone() for k, v in p.items()}, feats.double(), coords)
    net = net.to(dev())
    masks = []                                  # every ReLU in call order: the stand-alone one, then the block's two fused ones
    hook = net.relu.register_forward_hook(lambda m, i, o: masks.append((o.F.detach() > 0).cpu()))
    F_.set_relu_observer(lambda y: masks.append((y.detach() > 0).cpu()))
    try:
        logits = net(SparseTensor(feats.to(dev()), torch.from_numpy(coords).to(dev())))
    finally:
        F_.set_relu_observer(None)
        hook.remove()
    assert logits.shape == (2, 4) and len(masks) == 3
    e = rel_l2(logits, free)
    print("logits rel-L2 %.3e" % e)
    assert e <= 2e-4, "logits rel-L2 %.3e" % e
    ref = pr.pooled_net_forward(p, feats.double(), coords, relu_masks=masks)
    assert rel_l2(ref, free) <= 1e-6, "prescribing the fp32 activation pattern changed the float64 logits"
    torch.nn.functional.cross_entropy(ref, labels).backward()
    torch.nn.functional.cross_entropy(logits, labels.to(dev())).backward()
    worst = ("", 0.0)
    for name, prm in net.named_parameters():
        g = rel_l2(prm.grad, p[name].grad)
        if g > worst[1]:
            worst = (name, g)
    print("worst gradient %s rel-L2 %.3e" % worst)
    assert worst[1] <= 2e-4, "gradient of %s rel-L2 %.3e" % worst


def test_network_with_max_pooling_runs_and_repeats():
    from openscene_amd.sparse import SparseTensor
    coords, feats = scenes()
    labels = torch.tensor([1, 3], device=dev())
    runs = []
    for _ in range(2):
        net = build_net("max").to(dev())
        logits = net(SparseTensor(feats.to(dev()), torch.from_numpy(coords).to(dev())))
        torch.nn.functional.cross_entropy(logits, labels).backward()
        runs.append((logits.detach(), {k: v.grad.detach() for k, v in net.named_parameters()}))
    assert torch.isfinite(runs[0][0]).all()
    for name, g in runs[0][1].items():
        assert torch.isfinite(g).all() and float(g.abs().sum()) > 0, name
        same_bits(g, runs[1][1][name], name)
    same_bits(runs[0][0], runs[1][0], "logits")
