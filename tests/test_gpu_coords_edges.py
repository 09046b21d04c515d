"""The integer pipeline on the GPU where no other test takes it (cases and reasons: coords_edges.py; that they tell a right pipeline
from a wrong one: test_coords_edges_cpu.py) -- every comparison bit-exact against the oracle:

  past 2^20 rows     scan_sums_kernel's second and third chunk of block sums and the carry between them, the pyramid's grid of
                     more than 1024 blocks with the true count in device memory, rocPRIM's sort path above 1 M items; one test per
                     operation, the big inputs and their references built once per module (_CACHE)
  block boundaries   row counts at and beside the multiples of 64, 256 and 1024
  range              voxels on every face, edge and corner of the documented cube |c| <= 32766, scenes 0 and 65534; kernel offsets and
                     stride quantisation that step across the limit
  wrap               a hash cluster that runs from the last slots of the table over slot 0

The code accepts |c| = 32767 although the documents exclude it (|c| < 32767); that value is left unpinned here: no
case has a voxel there, and the rows that must raise start at 32768.
"""
import numpy as np
import pytest
import torch

from oracle import coords as oc
from oracle import loader as ol
from oracle import voxelize as ov

import coords_edges as ce
import cpu_backend

pytestmark = pytest.mark.gpu

STRIDES = (1, 2, 4, 8, 16)
_CACHE = {}


def dev():
    return torch.device("cuda", 0)


def _cached(name, fn):
    if name not in _CACHE:
        _CACHE[name] = fn()
    return _CACHE[name]


def _gpu(a):
    return torch.from_numpy(np.array(a)).to(dev())


def _big(name):
    """(rows as numpy, rows on the device) of coords_edges.big_cloud / big_duplicates, once per module."""
    return _cached(name, lambda: (getattr(ce, name)(), _gpu(getattr(ce, name)())))


def _ref_pyramid_big():
    return _cached("ref_pyramid", lambda: [tuple(t.numpy() for t in r[:3]) for r in cpu_backend.coords_pyramid(torch.from_numpy(np.array(ce.big_cloud())), STRIDES)])


def _manager_big():
    from openscene_amd.sparse import CoordinateManager
    return _cached("manager", lambda: CoordinateManager(_big("big_cloud")[1]))


def _eq(t, a):
    return np.array_equal(t.cpu().numpy(), np.asarray(a))


def _same3(a, b):
    return all(torch.equal(x, y) for x, y in zip(a[:3], b[:3]))


# ------------------------------------------------------------------------------------------------ past 2^20 rows
@pytest.mark.parametrize("name", ["big_cloud", "big_duplicates"])
def test_unique_past_2_20_rows(name):
    from openscene_amd import ops
    c, x = _big(name)
    assert c.shape[0] > 2 ** 20
    want = _ref_pyramid_big()[0] if name == "big_cloud" else tuple(t.numpy() for t in cpu_backend.coords_unique(torch.from_numpy(np.array(c)), 1)[:3])
    got = ops.coords_unique(x, 1)
    assert got[0].shape[0] == want[0].shape[0]
    for g, w, what in zip(got[:3], want, ("coordinates", "inverse", "first")):
        assert _eq(g, w), what
    u = got[0].shape[0]
    own = ops.kmap_build(got[3], got[0], 1, 1)                      # the table answers every unique row with its own number
    assert torch.equal(own, torch.arange(u, dtype=torch.int32, device=dev())[None])
    again = ops.coords_unique(x, 1)
    assert _same3(got, again) and torch.equal(ops.kmap_build(again[3], again[0], 1, 1), own)


def _check_pyramid(x, want):
    from openscene_amd import ops
    pyr = ops.coords_pyramid(x, STRIDES)
    assert [p[0].shape[0] for p in pyr] == [w[0].shape[0] for w in want]
    cur = x
    for s, p, w in zip(STRIDES, pyr, want):
        for g, ww, what in zip(p[:3], w, ("coordinates", "inverse", "first")):
            assert _eq(g, ww), "stride %d %s" % (s, what)
        chain = ops.coords_unique(cur, s)                            # the level-by-level chain
        assert _same3(p, chain), "stride %d" % s
        cur = chain[0]
    again = ops.coords_pyramid(x, STRIDES)
    assert all(_same3(a, b) for a, b in zip(pyr, again))
    return pyr


def test_pyramid_past_2_20_rows():
    """Level 0 above 2^20 rows, level 1 below it, every level on a grid of 1028 blocks with its count read from device memory."""
    want = _ref_pyramid_big()
    assert want[0][0].shape[0] == ce.N_BIG and want[1][0].shape[0] < 2 ** 20
    _check_pyramid(_big("big_cloud")[1], want)


def test_pyramid_past_2_20_rows_with_duplicates():
    """The same with the first 500 rows appended again.  The rows of big_cloud are distinct and the copies come last, so the reference
    follows from the one without them: the same unique rows at every level, the same `first`, and level 0's inverse = the row's own
    number, for the copies 0 .. 499."""
    c, x = _big("big_cloud")
    want = [tuple(w) for w in _ref_pyramid_big()]
    assert np.array_equal(want[0][0], c) and np.array_equal(want[0][1], np.arange(ce.N_BIG))
    want[0] = (want[0][0], np.concatenate([want[0][1], np.arange(500, dtype=np.int32)]), want[0][2])
    _check_pyramid(torch.cat([x, x[:500]]), want)


def test_manager_strided_maps_past_2_20_rows():
    """kmap(1, 2, 2), its transposed table and kmap(2, 1, 2) of CoordinateManager(big_cloud) against the oracle."""
    cm = _manager_big()
    ref = _ref_pyramid_big()
    assert [cm.size(s) for s in STRIDES] == [r[0].shape[0] for r in ref]
    assert _eq(cm.coords(2), ref[1][0]) and _eq(cm.parent(2), ref[1][1])
    want = oc.kernel_map(ref[0][0], ref[1][0], oc.kernel_offsets(2, 1))
    want_t = oc.transpose_table(want, ce.N_BIG)
    down, down_t, flip = cm.kmap(1, 2, 2)
    assert not flip and _eq(down, want) and _eq(down_t, want_t)
    up, up_t, flip = cm.kmap(2, 1, 2)
    assert not flip and _eq(up, want_t) and _eq(up_t, want)
    assert _eq(cm.kmap_counts(1, 2, 2), (want >= 0).sum(1)) and _eq(cm.kmap_counts(2, 1, 2), (want >= 0).sum(1))


def test_manager_3x3x3_map_past_2_20_rows():
    """kmap(1, 1, 3) of big_cloud: four of its offsets against the oracle (kmap_build has no path that depends on the row count beyond
    its indexing; the oracle's whole 27-offset map costs 13 s), the structure of a stride-1 map, the fused counts, both builders."""
    from openscene_amd import ops
    c, x = _big("big_cloud")
    cm = _manager_big()
    nbr, bwd, flip = cm.kmap(1, 1, 3)
    assert flip and bwd is nbr and nbr.shape == (27, ce.N_BIG)
    sub = [0, 5, 13, 26]
    assert _eq(nbr[sub], oc.kernel_map(c, c, oc.kernel_offsets(3, 1)[sub]))
    cnt = ops.kmap_count(nbr)
    assert torch.equal(cm.kmap_counts(1, 1, 3), cnt)                                   # fused count of kmap_build
    assert int(cnt[13]) == ce.N_BIG and torch.equal(cnt, torch.flip(cnt, dims=[0]))
    assert torch.equal(nbr[13], torch.arange(ce.N_BIG, dtype=torch.int32, device=dev()))
    assert torch.equal(ops.kmap_transpose(nbr, ce.N_BIG), torch.flip(nbr, dims=[0]))
    table = cm._tables[1]
    full, cf = ops.kmap_build(table, x, 3, 1, with_counts=True, self_map=False)
    half, ch = ops.kmap_build(table, x, 3, 1, with_counts=True, self_map=True)
    assert torch.equal(full, half) and torch.equal(cf, ch) and torch.equal(full, nbr) and torch.equal(cf, cnt)


def _sort_table(which):
    if which == "up_2x2x2":                                  # transposed 2^3 table of big_cloud: K = 8, one offset per row
        return _manager_big().kmap(2, 1, 2)[0]
    return _cached("synthetic27", lambda: _gpu(ce.synthetic_table(27, 2 ** 20 + 5, 0.3, 0)))


@pytest.mark.parametrize("with_counts", [False, True])
@pytest.mark.parametrize("which", ["up_2x2x2", "synthetic27"])
def test_kmap_sort_past_2_20_rows(which, with_counts):
    """n_out > 2^20: the sort path rocPRIM takes above 1 M items.  Many rows share a mask, so the order checks stability."""
    from openscene_amd import ops
    nbr = _sort_table(which)
    assert nbr.shape[1] > 2 ** 20
    cnt = ops.kmap_count(nbr) if with_counts else None
    host = nbr.cpu()
    assert cnt is None or torch.equal(cnt.cpu(), (host >= 0).sum(1))
    want = cpu_backend.kmap_sort(host, None if cnt is None else cnt.cpu())
    got = ops.kmap_sort(nbr, cnt)
    for g, w, what in zip(got, want, ("order", "table", "group masks")):
        assert torch.equal(g.cpu(), w), what
    assert all(torch.equal(a, b) for a, b in zip(got, ops.kmap_sort(nbr, cnt)))


def test_voxelize_past_2_20_points():
    """N_BIG float64 points in a box of 8 x 6 x 3 m at 2 cm: the voxeliser's scan over more than 1024 blocks."""
    from openscene_amd import ops
    rng = np.random.default_rng(20)
    xyz = rng.random((ce.N_BIG, 3)) * np.array([8.0, 6.0, 3.0]) - np.array([4.0, 3.0, 0.5])
    T = np.eye(4)
    np.fill_diagonal(T[:3, :3], 1 / 0.02)
    vox, inds, inverse = ov.voxelize_with_matrix(xyz, T)
    x = _gpu(xyz)
    grid, g_inds, g_inverse = ops.voxelize_fnv(x, T)
    assert g_inds.shape[0] == inds.shape[0]                                            # voxel count
    assert _eq(g_inds, inds) and _eq(g_inverse, inverse)
    grid_h = grid.cpu().numpy()
    want_grid = np.floor(xyz @ T[:3, :3].T)
    assert np.array_equal(grid_h, want_grid - want_grid.min(0)) and np.array_equal(grid_h[inds], vox)
    again = ops.voxelize_fnv(x, T)
    assert all(torch.equal(a, b) for a, b in zip((grid, g_inds, g_inverse), again))


def test_feature_remap_past_2_20_rows():
    """n_pts = N_BIG, n_vox = 2^20 + 9: both scans of the remap cross the threshold."""
    from openscene_amd import ops
    rng = np.random.default_rng(21)
    n_pts, n_vox = ce.N_BIG, 2 ** 20 + 9
    mask = rng.random(n_pts) < 0.55
    vox = rng.permutation(n_pts)[:n_vox].astype(np.int64)
    want = ol.remap(mask, vox)
    m, v = _gpu(mask), _gpu(vox)
    got = ops.feature_remap(m, v)
    for g, w, what in zip(got, want, ("mask_vox", "src_row", "indices")):
        assert g.shape[0] == np.asarray(w).shape[0] and _eq(g, w), what
    assert all(torch.equal(a, b) for a, b in zip(got, ops.feature_remap(m, v)))


def test_prebuild_past_2_20_rows(monkeypatch):
    """CoordinateManager.prebuild() of big_cloud through osn_maps_build (one stream): every neighbour table, transposed table, pair
    count and tile order equals what the per-map entry points give."""
    from openscene_amd import ops
    from openscene_amd.sparse import CoordinateManager
    x = _big("big_cloud")[1]
    monkeypatch.setattr(ops, "MAPS_STREAMS", 1)
    calls = []
    real = ops.maps_build
    monkeypatch.setattr(ops, "maps_build", lambda *a, **k: (calls.append(len(a[1])), real(*a, **k))[1])
    cm = CoordinateManager(x)
    cm.prebuild()
    assert calls == [10]
    ref = _manager_big()                                     # its maps come from kmap_build / kmap_transpose / kmap_sort one by one
    keys = [(1, 1, 5)] + [(s, s, 3) for s in STRIDES] + [(s, 2 * s, 2) for s in STRIDES[:-1]] + [(2 * s, s, 2) for s in STRIDES[:-1]]
    for key in keys:
        a, b = cm.kmap(*key), ref.kmap(*key)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2], key
        assert torch.equal(cm.kmap_counts(*key), ref.kmap_counts(*key)), key
        for ta, tb in zip(cm.kmap_tiles(*key), ref.kmap_tiles(*key)):
            assert (ta is None) == (tb is None), key
            if ta is not None:
                assert all(torch.equal(p, q) for p, q in zip(ta, tb)), key
    assert ref.kmap_tiles(1, 1, 3)[0] is not None and ref.kmap_tiles(1, 1, 3)[0][0].shape[0] == ce.N_BIG


# ------------------------------------------------------------------------------------------------ block boundaries
@pytest.mark.parametrize("n,last", ce.boundary_cases())
def test_unique_at_the_block_boundaries(n, last):
    from openscene_amd import ops
    c = ce.boundary_cloud(n, last)
    x = _gpu(c)
    for s in (1, 2):
        want = cpu_backend.coords_unique(torch.from_numpy(c), s)
        got = ops.coords_unique(x, s)
        for g, w, what in zip(got[:3], want[:3], ("coordinates", "inverse", "first")):
            assert g.shape == w.shape and torch.equal(g.cpu(), w), (s, what)
        assert _same3(got, ops.coords_unique(x, s))
    if n >= 1023:
        want = cpu_backend.coords_pyramid(torch.from_numpy(c), STRIDES)
        got = ops.coords_pyramid(x, STRIDES)
        for s, g, w in zip(STRIDES, got, want):
            assert all(a.shape == b.shape and torch.equal(a.cpu(), b) for a, b in zip(g[:3], w[:3])), s
        assert all(_same3(a, b) for a, b in zip(got, ops.coords_pyramid(x, STRIDES)))


# ------------------------------------------------------------------------------------------------ range
def _range_levels():
    def make():
        from openscene_amd import ops
        c = ce.range_cloud()
        x = _gpu(c)
        want = cpu_backend.coords_pyramid(torch.from_numpy(np.array(c)), (1, 2))
        pyr = ops.coords_pyramid(x, (1, 2))
        return x, want, pyr
    return _cached("range_levels", make)


def test_range_cloud_unique_and_pyramid():
    from openscene_amd import ops
    x, want, pyr = _range_levels()
    for g, w in zip(pyr, want):
        assert all(a.shape == b.shape and torch.equal(a.cpu(), b) for a, b in zip(g[:3], w[:3]))
    cur = x
    for s, w in zip((1, 2), want):
        got = ops.coords_unique(cur, s)
        assert all(a.shape == b.shape and torch.equal(a.cpu(), b) for a, b in zip(got[:3], w[:3])), s
        cur = got[0]
    got2 = ops.coords_unique(x, 2)                                    # stride 2 straight from the input rows
    want2 = cpu_backend.coords_unique(torch.from_numpy(np.array(ce.range_cloud())), 2)
    assert all(a.shape == b.shape and torch.equal(a.cpu(), b) for a, b in zip(got2[:3], want2[:3]))


@pytest.mark.parametrize("scale", [1, 2])
@pytest.mark.parametrize("ksize", ce.KSIZES)
def test_range_cloud_kernel_maps(ksize, scale):
    """Maps over the voxels at the limit: hits next to every face, probes that leave the packable range refused (masked oracle:
    coords_edges.masked_kernel_map); both builders for the odd sizes; the fused counts."""
    from openscene_amd import ops
    x, want, pyr = _range_levels()
    lvl = scale - 1
    coords, _, _, table = pyr[lvl]
    ref_c = want[lvl][0].numpy()
    ref = ce.masked_kernel_map(ref_c, ref_c, ksize, scale)
    reach = (ksize // 2 if ksize & 1 else ksize - 1) * scale             # probes leave [-32767, 32767] from 32766 once they reach 2 cells
    assert bool(ce.probe_out_of_range(ref_c, ksize, scale).any()) == (reach >= 2) and (ref >= 0).sum() > ref_c.shape[0]
    builders = (False, True) if ksize & 1 else (False,)
    for self_map in builders:
        nbr, cnt = ops.kmap_build(table, coords, ksize, scale, with_counts=True, self_map=self_map)
        assert _eq(nbr, ref), self_map
        assert _eq(cnt, (ref >= 0).sum(1)), self_map
        assert torch.equal(ops.kmap_build(table, coords, ksize, scale, self_map=self_map), nbr)
    if ksize == 2 and scale == 1:                                     # the strided map level 0 -> level 1
        ref_o = want[1][0].numpy()
        down = ops.kmap_build(table, pyr[1][0], 2, 1)
        assert _eq(down, ce.masked_kernel_map(ref_c, ref_o, 2, 1))
        assert _eq(ops.kmap_transpose(down, coords.shape[0]), oc.transpose_table(ce.masked_kernel_map(ref_c, ref_o, 2, 1), ref_c.shape[0]))


@pytest.mark.parametrize("case", ce.range_raises(), ids=[r[0] for r in ce.range_raises()])
def test_rows_past_the_range_raise(case):
    """|c| = 32768 in any column, -32767 at stride 2 (quantised to -32768) and scene 65535: coords_unique and coords_pyramid raise."""
    from openscene_amd import ops
    from openscene_amd._lib import OpenSceneAmdError
    _, c, strides = case
    x = _gpu(c)
    for s in strides:
        with pytest.raises(OpenSceneAmdError):
            ops.coords_unique(x, s)
    with pytest.raises(OpenSceneAmdError):
        ops.coords_pyramid(x, (1, 2))
    with pytest.raises(OpenSceneAmdError):
        ops.coords_pyramid(x, STRIDES)


# ------------------------------------------------------------------------------------------------ wrap
def test_hash_cluster_wraps_over_slot_0():
    """coords_unique(wrap_cloud), the table read back: the occupied slots are the model's (that set does not depend on the insertion
    order), slots cap - 1 and 0 hold keys homed at >= cap - 3, every key's value is its unique row; the 3^3 map over it is the oracle's."""
    from openscene_amd import ops
    w = ce.wrap_cloud()
    x = _gpu(w.rows)
    for _ in range(2):
        out, inv, first, table = ops.coords_unique(x, 1)
        assert table.cap == w.cap and _eq(out, w.rows) and _eq(inv, np.arange(w.rows.shape[0]))
        keys = table.keys.cpu().numpy().view(np.uint64)
        vals = table.vals.cpu().numpy()
        occ = keys != ce.KEY_EMPTY
        assert np.array_equal(occ, w.occupied)
        home = ce.hash_key(keys) & (w.cap - 1)
        assert occ[w.cap - 1] and occ[0] and home[w.cap - 1] >= w.cap - 3 and home[0] >= w.cap - 3
        row_of = {int(k): i for i, k in enumerate(ce.pack_key(w.rows))}
        assert sorted(int(k) for k in keys[occ]) == sorted(row_of)
        assert all(int(vals[s]) == row_of[int(keys[s])] for s in np.nonzero(occ)[0])
        nbr = ops.kmap_build(table, out, 3, 1)
        assert _eq(nbr, oc.kernel_map(w.rows, w.rows, oc.kernel_offsets(3, 1)))
        assert torch.equal(ops.kmap_build(table, out, 3, 1, self_map=True), nbr)
