"""Sparse pooling layers without a GPU: the laws of the numpy restatement the GPU tests compare against
(tests/pooling_reference.py), the MinkowskiEngine names and parameter keys of the modules, the module tree on the mock
library (how many C calls a forward + backward makes), and the argument checks of every new C entry."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import cpu_backend
import pooling_reference as pr
from oracle import coords as oc

MAPS = [("k3s1", 3, 1), ("k2s2", 2, 2), ("k3s2", 3, 2)]       # the mirror path, and two transposed-table paths


def occupancy(seed, side=6, p=0.4):
    rng = np.random.default_rng(seed)
    g = np.argwhere(rng.random((side, side, side)) < p).astype(np.int32)
    g = g[rng.permutation(g.shape[0])]
    return np.concatenate([np.zeros((g.shape[0], 1), np.int32), g], 1)


def geometry(ksize, stride, seed=0):
    fine = occupancy(seed)
    out = fine if stride == 1 else oc.stride_map(fine, stride)[0]
    return fine, out, pr.tables(fine, out, ksize)


# ---- the reference's own laws ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,ksize,stride", MAPS)
def test_sum_of_ones_is_the_count_and_avg_keeps_a_constant(name, ksize, stride):
    fine, out, (nbr, nbr_bwd, flip) = geometry(ksize, stride)
    assert flip == (name == "k3s1") and (nbr_bwd is nbr) == flip
    ones = np.ones((fine.shape[0], 3), np.float32)
    y, _, cnt = pr.local_fwd(ones, nbr, "sum")
    assert cnt.min() >= 1 and cnt.max() > cnt.min()
    assert np.array_equal(y, np.repeat(cnt[:, None], 3, 1).astype(np.float32))
    for const in (1.5, -0.375):                 # k * const is exact for every k <= 27: the quotient is the constant itself
        y, _, _ = pr.local_fwd(ones * np.float32(const), nbr, "avg")
        assert np.array_equal(y.view(np.int32), np.full_like(y, const).view(np.int32))


@pytest.mark.parametrize("mode", ["sum", "avg", "max"])
@pytest.mark.parametrize("name,ksize,stride", MAPS)
def test_backward_is_the_transpose_of_forward(name, ksize, stride, mode):
    """<gy, P x> = <P^T gy, x>; integer-valued operands make every float32 sum exact, so sum and max hold exactly."""
    fine, out, (nbr, nbr_bwd, flip) = geometry(ksize, stride, seed=1)
    rng = np.random.default_rng(2)
    x = rng.integers(-8, 9, (fine.shape[0], 5)).astype(np.float32)
    gy = rng.integers(-8, 9, (out.shape[0], 5)).astype(np.float32)
    y, arg, cnt = pr.local_fwd(x, nbr, mode)
    gx = pr.local_bwd(gy, nbr_bwd, flip, mode, cnt=cnt, arg=arg)
    lhs, rhs = float((gy.astype(np.float64) * y).sum()), float((gx.astype(np.float64) * x).sum())
    if mode == "avg":
        assert abs(lhs - rhs) <= 1e-5 * float((np.abs(gy.astype(np.float64)) * np.abs(y)).sum())
    else:
        assert lhs == rhs


@pytest.mark.parametrize("name,ksize,stride", MAPS)
def test_tables_agree_with_the_dense_float64_restatement(name, ksize, stride):
    """The mirror path (k3s1) and the transposed-table paths (k2s2, k3s2) against an operator built from the coordinates alone."""
    fine, out, (nbr, nbr_bwd, flip) = geometry(ksize, stride, seed=3)
    P = pr.dense_operator(fine, out, ksize)
    rng = np.random.default_rng(4)
    x = rng.standard_normal((fine.shape[0], 4)).astype(np.float32)
    gy = rng.standard_normal((out.shape[0], 4)).astype(np.float32)
    n = P.sum(1, keepdims=True)
    for mode, want_y, want_gx in (("sum", P @ x, P.T @ gy), ("avg", P @ x / n, P.T @ (gy / n))):
        y, _, cnt = pr.local_fwd(x, nbr, mode)
        assert np.array_equal(cnt, n[:, 0].astype(np.int32))
        gx = pr.local_bwd(gy, nbr_bwd, flip, mode, cnt=cnt)
        np.testing.assert_allclose(y, want_y, rtol=0, atol=1e-5)
        np.testing.assert_allclose(gx, want_gx, rtol=0, atol=1e-5)
    y, arg, _ = pr.local_fwd(x, nbr, "max")
    want = np.where(P[:, :, None] > 0, x[None].astype(np.float64), -np.inf)
    assert np.array_equal(y, want.max(1).astype(np.float32)) and np.array_equal(arg, want.argmax(1))
    gx = pr.local_bwd(gy, nbr_bwd, flip, "max", arg=arg)
    want_gx = np.zeros_like(gx, dtype=np.float64)
    np.add.at(want_gx, (arg, np.arange(4)[None]), gy)
    np.testing.assert_allclose(gx, want_gx, rtol=0, atol=1e-5)


def test_max_rules_of_the_reference():
    nbr = np.array([[0], [1], [2], [-1]], np.int32)
    x = np.array([[1.0, 0.0, np.nan, -np.inf], [1.0, -0.0, 5.0, -np.inf], [0.5, 0.0, np.nan, -np.inf]], np.float32)
    y, arg, cnt = pr.local_fwd(x, nbr, "max")
    assert cnt[0] == 3 and arg.tolist() == [[0, 0, 0, 0]]
    assert y[0, 0] == 1.0 and not np.signbit(y[0, 1]) and np.isnan(y[0, 2]) and y[0, 3] == -np.inf
    y, arg, _ = pr.local_fwd(x[::-1].copy(), nbr, "max")        # rows 2, 1, 0: the NaN of k = 0 stays, -0 comes after +0
    assert arg.tolist() == [[1, 0, 0, 0]] and not np.signbit(y[0, 1])
    gy, garg, _ = pr.global_fwd64(x, np.zeros(3, np.int64), "max")
    assert garg.tolist() == [[0, 0, 0, 0]]


def test_global_reference_orders_batches_and_rows():
    b = np.array([5, 0, 2, 5, 0, 5])
    x = np.arange(12, dtype=np.float32).reshape(6, 2)
    y, _, counts = pr.global_fwd64(x, b, "sum")
    assert counts.tolist() == [2, 1, 3] and y.tolist() == [[2 + 8, 3 + 9], [4, 5], [0 + 6 + 10, 1 + 7 + 11]]
    y, arg, _ = pr.global_fwd64(x, b, "max")
    assert arg.tolist() == [[4, 4], [2, 2], [5, 5]]
    gx = pr.global_bwd(np.ones((3, 2), np.float32), b, "avg")
    assert gx[:, 0].tolist() == [np.float32(1) / np.float32(3), 0.5, 1.0, np.float32(1) / np.float32(3), 0.5, np.float32(1) / np.float32(3)]
    assert pr.global_bwd(np.ones((3, 2), np.float32), b, "max", arg=arg).sum() == 6


# ---- the modules ----------------------------------------------------------------------------------------------------------------
def test_modules_construct_and_carry_me_names():
    from openscene_amd import minkowski as me
    assert set(me.MinkowskiLinear(8, 4).state_dict()) == {"linear.weight", "linear.bias"}
    assert set(me.MinkowskiLinear(8, 4, bias=False).state_dict()) == {"linear.weight"}
    assert tuple(me.MinkowskiLinear(8, 4).linear.weight.shape) == (4, 8)

    class Head(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.glob_avg = me.MinkowskiGlobalMaxPooling()
            self.final = me.MinkowskiLinear(8, 4)
    assert set(Head().state_dict()) == {"final.linear.weight", "final.linear.bias"}
    for cls in (me.MinkowskiSumPooling, me.MinkowskiAvgPooling, me.MinkowskiMaxPooling):
        m = cls(kernel_size=2, stride=2, dimension=3)
        assert (m.kernel_size, m.stride, m.dilation, m.kernel_volume) == (2, 2, 1, 8) and not list(m.parameters())
        assert cls(3).stride == 1 and cls(3).kernel_volume == 27
        with pytest.raises(NotImplementedError):
            cls(3, stride=3)
        with pytest.raises(NotImplementedError):
            cls(5)
        with pytest.raises(NotImplementedError):
            cls((2, 2, 3))
        with pytest.raises(NotImplementedError):
            cls(2, dimension=4)
    for cls in (me.MinkowskiGlobalSumPooling, me.MinkowskiGlobalAvgPooling, me.MinkowskiGlobalMaxPooling,
                me.MinkowskiBroadcastAddition, me.MinkowskiBroadcastMultiplication):
        assert not list(cls().parameters())


def test_alias_exports_the_pooling_names():
    import openscene_amd
    src = open(os.path.join(ROOT, "openscene_amd", "__init__.py")).read()
    from openscene_amd import minkowski as me
    for name in ("MinkowskiSumPooling", "MinkowskiAvgPooling", "MinkowskiMaxPooling", "MinkowskiGlobalSumPooling",
                 "MinkowskiGlobalAvgPooling", "MinkowskiGlobalMaxPooling", "MinkowskiBroadcastAddition",
                 "MinkowskiBroadcastMultiplication", "MinkowskiLinear"):
        assert '"%s"' % name in src and issubclass(getattr(me, name), torch.nn.Module)
    assert openscene_amd.install_minkowski_alias is not None


# ---- the module tree on the mock library (the fixture pattern of tests/test_mock_abi.py) ----------------------------------
@pytest.fixture()
def mock_ops(monkeypatch):
    import host_profile
    from openscene_amd import _lib, ops
    mock = host_profile.build_mock()
    calls = {}

    class Counting:
        """Counts calls per entry point; ctypes still checks every argument against the prototype."""

        def __getattr__(self, name):
            fn = getattr(mock, name)

            def wrapped(*a):
                calls[name] = calls.get(name, 0) + 1
                return fn(*a)
            return wrapped

    lib = Counting()
    monkeypatch.setattr(_lib, "_lib", lib)
    monkeypatch.setattr(_lib, "require_device", lambda dev: None)
    monkeypatch.setattr(ops, "_prep", lambda dev: lib)
    monkeypatch.setattr(ops, "_stream", lambda dev: None)
    monkeypatch.setattr(ops, "_idx", lambda dev: 0)
    monkeypatch.setattr(ops, "_tl_counters", {})
    monkeypatch.setattr(ops, "_ws", lambda nbytes, dev: torch.empty(max(int(nbytes), 16), dtype=torch.uint8))
    monkeypatch.setattr(ops, "_size_cache", {})
    monkeypatch.setattr(ops, "_plan_cache", {})

    class NoDev:
        def __init__(self, dev):
            pass

        def __enter__(self):
            pass

        def __exit__(self, *a):
            pass
    monkeypatch.setattr(ops, "_Dev", NoDev)
    for n in ("HashTable", "coords_unique", "coords_pyramid", "kmap_build", "kmap_transpose", "kmap_sort", "kmap_count"):
        monkeypatch.setattr(ops, n, getattr(cpu_backend, n))
    return calls


def test_module_tree_runs_on_the_mock_library(mock_ops):
    from openscene_amd import minkowski as me
    from openscene_amd import ops
    from openscene_amd import synthetic as syn
    from openscene_amd.sparse import ORIGIN_STRIDE, SparseTensor
    ops.clear_weight_cache()

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.conv = me.MinkowskiConvolution(3, 8, kernel_size=3, dimension=3)
            self.avg = me.MinkowskiAvgPooling(2, 2)
            self.max = me.MinkowskiMaxPooling(3)
            self.sum = me.MinkowskiSumPooling(3, 2)
            self.gavg, self.gmax, self.gsum = me.MinkowskiGlobalAvgPooling(), me.MinkowskiGlobalMaxPooling(), me.MinkowskiGlobalSumPooling()
            self.se = me.MinkowskiLinear(8, 8)
            self.gate, self.shift = me.MinkowskiBroadcastMultiplication(), me.MinkowskiBroadcastAddition()
            self.final = me.MinkowskiLinear(8, 4)

        def forward(self, x):
            x = self.sum(self.max(self.avg(self.conv(x))))
            x = self.gate(x, self.se(self.gavg(x)))
            x = self.shift(x, self.gsum(x))
            return self.final(self.gmax(x))

    torch.manual_seed(0)
    net = Net()
    vox = [syn.shuffled(syn.grid_voxels(syn.room_points(s, n_pts=3000), 0.1), s) for s in (0, 1)]
    coords = torch.from_numpy(syn.batch_coords(vox))
    x = SparseTensor(torch.ones(coords.shape[0], 3), coords)
    mock_ops.clear()
    out = net(x)
    assert out.shape == (2, 4) and out.tensor_stride == ORIGIN_STRIDE and out.coordinate_manager is x.coordinate_manager
    assert out.C.tolist() == [[0, 0, 0, 0], [1, 0, 0, 0]] and out.C.dtype == torch.int32
    out.F.sum().backward()
    c = dict(mock_ops)
    # one launch per local pooling and direction; the average's divisor once per map
    assert c.get("osn_pool_fwd") == 3 and c.get("osn_pool_bwd") == 3 and c.get("osn_pool_count") == 1, c
    # three global poolings; the broadcast pair: two forwards, the multiplication's streaming input gradient, two pooled gradients
    assert c.get("osn_gpool_fwd") == 3 and c.get("osn_gpool_bwd") == 3, c
    assert c.get("osn_broadcast_fwd") == 3 and c.get("osn_broadcast_bwd_pooled") == 2, c
    assert all(p.grad is not None for p in net.parameters())
    # a second pass builds nothing again: the divisor and the batch index are cached on the manager
    mock_ops.clear()
    net(x)
    assert "osn_pool_count" not in mock_ops and mock_ops.get("osn_pool_fwd") == 3, dict(mock_ops)
    cm = x.coordinate_manager
    idx = cm.batch_index(4)
    assert idx is cm.batch_index(4) and idx.ids.tolist() == [0, 1] and idx.offsets.dtype == torch.int64
    # both live in the cache CoordinateManager.tensors() / record_stream() walk (the walk itself: test_gpu_pooling.py)
    assert cm._kmaps[("batch", 4)] is idx and cm._kmaps[("pool_cnt", 1, 2, 2, 1)] is cm.pool_counts(1, 2, 2)
    # a pooled tensor goes through the feature-only layers, and is refused where a kernel map is needed
    pooled = me.MinkowskiGlobalAvgPooling()(net.conv(x))
    assert me.cat(pooled, pooled).shape == (2, 16) and (pooled + pooled).shape == (2, 8)
    for layer in (me.MinkowskiConvolution(8, 8, kernel_size=3, dimension=3), me.MinkowskiConvolution(8, 8, kernel_size=1, dimension=3),
                  me.MinkowskiMaxPooling(2, 2), me.MinkowskiGlobalSumPooling()):
        with pytest.raises(ValueError):
            layer(pooled)
    ops.clear_weight_cache()


def test_batch_index_allows_gaps_and_interleaved_rows(mock_ops):
    from openscene_amd.sparse import CoordinateManager
    b = [5, 0, 2, 5, 0, 5]
    coords = torch.tensor([[v, i, 0, 0] for i, v in enumerate(b)], dtype=torch.int32)
    idx = CoordinateManager(coords).batch_index(1)
    assert idx.ids.tolist() == [0, 2, 5] and idx.rank.tolist() == [2, 0, 1, 2, 0, 2]
    assert idx.order.tolist() == [1, 4, 2, 0, 3, 5] and idx.offsets.tolist() == [0, 2, 3, 6]
    assert all(t.dtype == torch.int32 for t in (idx.ids, idx.rank, idx.order))


# ---- argument checks of the C entries: -1 (OSN_E_ARG), the entry's name first, nothing launched -----------------------------
def test_pooling_entries_argument_errors():
    import __graft_entry__ as ge
    ge.build()
    from openscene_amd import _lib, ops
    h = _lib.load()
    assert ops.GPOOL_CHUNK == 512 and ops.GPOOL_CHUNK <= 512
    n, c, K, B = 8, 16, 8, 2
    ws_bytes = h.osn_gpool_ws_bytes(n, B, c)
    assert ws_bytes >= (B + 1) * 8 + 2 * (n // ops.GPOOL_CHUNK + B) * c * 4
    buf = (ctypes.c_char * (8192 + ws_bytes + 16))()
    p = (ctypes.addressof(buf) + 15) & ~15
    x, y, tbl, arg, cnt, ws = p, p + 1024, p + 2048, p + 3072, p + 4096, p + 8192

    def refused(name, rc):
        assert rc == -1, (name, rc)
        assert _lib.last_error().startswith(name + ":"), _lib.last_error()

    def count(**kw):
        a = dict(nbr=tbl, n_in=n, n_out=n, K=K, cnt=cnt)
        a.update(kw)
        return h.osn_pool_count(a["nbr"], a["n_in"], a["n_out"], a["K"], a["cnt"], None)
    for bad in (dict(nbr=None), dict(cnt=None), dict(K=0), dict(K=9), dict(K=28), dict(n_out=-1)):
        refused("osn_pool_count", count(**bad))

    def fwd(**kw):
        a = dict(x=x, n_in=n, nbr=tbl, n_out=n, K=K, c=c, mode=0, y=y, arg=arg)
        a.update(kw)
        return h.osn_pool_fwd(a["x"], a["n_in"], a["nbr"], a["n_out"], a["K"], a["c"], a["mode"], a["y"], a["arg"], None)
    for bad in (dict(x=None), dict(nbr=None), dict(y=None), dict(mode=2, arg=None), dict(K=0), dict(K=9), dict(K=28), dict(mode=3), dict(mode=-1),
                dict(c=0)):
        refused("osn_pool_fwd", fwd(**bad))

    def bwd(**kw):
        a = dict(gy=y, n_out=n, nbr=tbl, n_in=n, K=K, flip=0, c=c, mode=0, cnt=cnt, arg=arg, gx=x)
        a.update(kw)
        return h.osn_pool_bwd(a["gy"], a["n_out"], a["nbr"], a["n_in"], a["K"], a["flip"], a["c"], a["mode"], a["cnt"], a["arg"], a["gx"], None)
    for bad in (dict(gy=None), dict(nbr=None), dict(gx=None), dict(mode=1, cnt=None), dict(mode=2, arg=None), dict(K=0), dict(K=9), dict(K=28),
                dict(mode=3), dict(flip=2)):
        refused("osn_pool_bwd", bwd(**bad))

    def gfwd(**kw):
        a = dict(x=x, n=n, c=c, order=tbl, offsets=cnt, B=B, mode=0, y=y, arg=arg, ws=ws, ws_bytes=ws_bytes)
        a.update(kw)
        return h.osn_gpool_fwd(a["x"], a["n"], a["c"], a["order"], a["offsets"], a["B"], a["mode"], a["y"], a["arg"], a["ws"], a["ws_bytes"], None)
    for bad in (dict(x=None), dict(order=None), dict(offsets=None), dict(y=None), dict(mode=2, arg=None), dict(mode=3), dict(c=0),
                dict(ws=None), dict(ws_bytes=ws_bytes - 1), dict(ws_bytes=0)):
        refused("osn_gpool_fwd", gfwd(**bad))

    def gbwd(**kw):
        a = dict(gy=y, rank=tbl, offsets=cnt, arg=arg, n=n, B=B, c=c, mode=0, gx=x)
        a.update(kw)
        return h.osn_gpool_bwd(a["gy"], a["rank"], a["offsets"], a["arg"], a["n"], a["B"], a["c"], a["mode"], a["gx"], None)
    for bad in (dict(gy=None), dict(rank=None), dict(gx=None), dict(mode=1, offsets=None), dict(mode=2, arg=None), dict(mode=3), dict(n=-1)):
        refused("osn_gpool_bwd", gbwd(**bad))

    def bfwd(**kw):
        a = dict(x=x, g=y, rank=tbl, n=n, B=B, c=c, op=0, y=p + 5120)
        a.update(kw)
        return h.osn_broadcast_fwd(a["x"], a["g"], a["rank"], a["n"], a["B"], a["c"], a["op"], a["y"], None)
    for bad in (dict(x=None), dict(g=None), dict(rank=None), dict(y=None), dict(op=2), dict(op=-1), dict(c=0)):
        refused("osn_broadcast_fwd", bfwd(**bad))

    def bbwd(**kw):
        a = dict(gy=y, x=x, n=n, c=c, order=tbl, offsets=cnt, B=B, gg=p + 5120, ws=ws, ws_bytes=ws_bytes)
        a.update(kw)
        return h.osn_broadcast_bwd_pooled(a["gy"], a["x"], a["n"], a["c"], a["order"], a["offsets"], a["B"], a["gg"], a["ws"], a["ws_bytes"], None)
    for bad in (dict(gy=None), dict(order=None), dict(offsets=None), dict(gg=None), dict(ws_bytes=16), dict(ws=None), dict(n=-1)):
        refused("osn_broadcast_bwd_pooled", bbwd(**bad))
    # sizes that need no launch are accepted without touching a pointer
    assert fwd(n_out=0, x=None, nbr=None, y=None) == 0 and gfwd(B=0, x=None, y=None, ws=None, ws_bytes=0) == 0 and bfwd(n=0, x=None) == 0
