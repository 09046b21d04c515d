"""openscene_amd.neighbors on the device against the numpy restatement of tests/neighbors_reference.py.  The search and the
vote are compared bit for bit; the blend bit for bit where the mean is exact and against the float64 formula within the bound
of neighbors_reference.blend_bound otherwise.  Every device result is computed twice and must repeat bit for bit."""
import functools

import numpy as np
import pytest
import torch

import neighbors_reference as nr

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def case(name):
    return getattr(nr, name + "_case")()


@functools.lru_cache(maxsize=None)
def index_of(name):
    from openscene_amd.neighbors import PointIndex
    from openscene_amd.objects import VoxelGrid
    c = case(name)
    return PointIndex(VoxelGrid(torch.from_numpy(c["xyz"]).to(dev()), c["offsets"], voxel_size=c["voxel_size"]))


@functools.lru_cache(maxsize=None)
def ref_knn(name, k):
    c = case(name)
    return nr.knn(c["xyz"], c["offsets"], c["voxel_size"], c["queries"], c["qscene"], k, c["radius"])


def bits(t):
    a = t.cpu().numpy()
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def twice(f):
    """f() -> tensors; called twice, the two results equal bit for bit -> the first."""
    a, b = f(), f()
    for x, y in zip(a, b):
        assert np.array_equal(bits(x), bits(y))
    return a


def same(got, ref):
    idx, dist, count = ref
    assert np.array_equal(got[2].cpu().numpy(), count)
    assert np.array_equal(got[0].cpu().numpy(), idx)
    assert np.array_equal(bits(got[1]), dist.view(np.uint32))


def knn_of(name, k, index=None, **kw):
    c = case(name)
    index = index_of(name) if index is None else index
    q, s = torch.from_numpy(c["queries"]).to(dev()), torch.from_numpy(c["qscene"]).to(dev())
    return twice(lambda: tuple(index.knn(q, k, radius=c["radius"], scene=s, **kw)))


# ---------------------------------------------------------------------------------------------------- the search
@pytest.mark.parametrize("k", [1, 4, 5, 16])
def test_lattice_with_ties_faces_and_points_at_the_radius(k):
    same(knn_of("lattice", k), ref_knn("lattice", k))


@pytest.mark.parametrize("k", [4, 16])
def test_a_crowded_cell_and_a_query_with_two_candidates(k):
    got = knn_of("crowded", k)
    same(got, ref_knn("crowded", k))
    assert got[2].tolist()[0] == k and got[2].tolist()[3] == 2 and (got[0][3, 2:] == -1).all() and torch.isinf(got[1][3, 2:]).all()


def test_two_scenes_with_the_same_coordinates_never_mix():
    got = knn_of("two_scene", 8)
    same(got, ref_knn("two_scene", 8))
    idx = got[0].cpu()
    assert ((idx[:64] < 150).all()) and ((idx[64:] == -1) | (idx[64:] >= 150)).all() and int(got[2].min()) >= 1


def test_queries_without_neighbours_and_invalid_queries_get_count_zero():
    got = knn_of("empty", 4)
    same(got, ref_knn("empty", 4))
    assert got[2].tolist()[:-1] == [0] * 8 and got[2].tolist()[-1] > 0


def test_exclude_knn_self_and_a_sources_mask():
    from openscene_amd.neighbors import PointIndex
    c = case("lattice")
    grid = index_of("lattice").grid
    n = c["xyz"].shape[0]
    mask = np.random.default_rng(1).random(n) < 0.3                       # (empties some cells)
    own, scene = np.arange(n, dtype=np.int32), np.zeros(n, dtype=np.int64)
    ex = np.random.default_rng(2).integers(0, n, c["queries"].shape[0]).astype(np.int32)
    emptied = 0
    for sources in (None, mask):
        index = index_of("lattice") if sources is None else PointIndex(grid, torch.from_numpy(sources).to(dev()))
        if sources is not None:
            emptied = int((index.cell_start[1:] == index.cell_start[:-1]).sum())
        same(twice(lambda: tuple(index.knn_self(4))), nr.knn(c["xyz"], c["offsets"], 1.0, c["xyz"], scene, 4, 1.0, sources=sources))
        same(twice(lambda: tuple(index.knn_self(4, include_self=False))),
             nr.knn(c["xyz"], c["offsets"], 1.0, c["xyz"], scene, 4, 1.0, sources=sources, exclude=own))
        same(knn_of("lattice", 4, index=index, exclude=torch.from_numpy(ex).to(dev())),
             nr.knn(c["xyz"], c["offsets"], 1.0, c["queries"], c["qscene"], 4, 1.0, sources=sources, exclude=ex))
    assert emptied > 0


@pytest.mark.parametrize("m", [0, 1, 63, 65, 257])
def test_query_counts_around_the_wave_and_the_block(m):
    c = case("random")
    ref = ref_knn("random", 8)
    q, s = torch.from_numpy(c["queries"][:m]).to(dev()), torch.from_numpy(c["qscene"][:m]).to(dev())
    got = twice(lambda: tuple(index_of("random").knn(q, 8, scene=s)))
    same(got, tuple(r[:m] for r in ref))
    assert got[0].shape == (m, 8) and got[2].shape == (m,)


def test_a_grid_without_points():
    from openscene_amd.neighbors import PointIndex
    from openscene_amd.objects import VoxelGrid
    index = PointIndex(VoxelGrid(torch.zeros((0, 3), device=dev()), None, voxel_size=0.1))
    got = twice(lambda: tuple(index.knn(torch.rand((65, 3), device=dev()), 3)))
    assert (got[2] == 0).all() and (got[0] == -1).all() and torch.isinf(got[1]).all()
    got = tuple(index.knn_self(3))
    assert got[0].shape == (0, 3) and got[2].shape == (0,)


def test_the_random_case():
    got = knn_of("random", 8)
    same(got, ref_knn("random", 8))
    count = got[2].cpu().numpy()
    assert (count == 8).any() and ((count > 0) & (count < 8)).any() and (count >= 1).sum() * 2 >= count.shape[0]


def test_entries_out_of_range_are_skipped_and_recorded():
    from openscene_amd import _lib, ops
    index = index_of("lattice")
    g = index.grid
    n, v = g.n_points, g.n_voxels
    zero = lambda: torch.zeros(1, dtype=torch.int32, device=dev())

    def search(err=None, cell_start=index.cell_start, cell_points=index.cell_points, nbr=g.nbr, q_cell=g.inverse, order=None):
        return ops.knn_grid(g.xyz, cell_start, cell_points, nbr, g.xyz, q_cell, 4, 1.0, order=order, err=err)

    def edited(t, at, value):
        t = t.clone()
        t[at] = value
        return t

    idx, dist2, count = search()
    arange = torch.arange(n, dtype=torch.int32, device=dev())
    cases = [(dict(cell_points=edited(index.cell_points, 5, n + 7)), ops.KNN_E_POINT), (dict(cell_points=edited(index.cell_points, 9, -2)), ops.KNN_E_POINT),
             (dict(cell_start=edited(index.cell_start, 3, n + 1)), ops.KNN_E_POINT), (dict(nbr=edited(g.nbr, (3, 2), v + 1)), ops.KNN_E_CELL),
             (dict(q_cell=edited(g.inverse, 0, v)), ops.KNN_E_CELL), (dict(q_cell=edited(g.inverse, 0, -2)), ops.KNN_E_CELL),
             (dict(order=edited(arange, 7, n)), ops.KNN_E_ORDER)]
    for kw, bit in cases:
        err = zero()
        got = search(err=err, **kw)
        assert int(err) == bit, (kw.keys(), int(err))
        if "order" not in kw:                                               # (a query no order entry names is not written)
            assert int(got[0].max()) < n and int(got[0].min()) >= -1         # nothing out of range comes back
        with pytest.raises(_lib.OpenSceneAmdError):
            search(**kw)
    values = torch.from_numpy(case("lattice")["values"]).to(dev())
    labels = torch.from_numpy(case("lattice")["labels"]).to(dev())
    for bad_idx, bad_count in ((edited(idx, (2, 0), n), count), (edited(idx, (2, 0), -1), count), (idx, edited(count, 4, 5)), (idx, edited(count, 4, -1))):
        err = zero()
        ops.knn_blend(values, bad_idx, dist2, bad_count, err=err)
        assert int(err) == ops.KNN_E_NEIGHBOR
        err = zero()
        ops.knn_vote(labels, bad_idx, bad_count, err=err)
        assert int(err) == ops.KNN_E_NEIGHBOR
        with pytest.raises(_lib.OpenSceneAmdError):
            ops.knn_blend(values, bad_idx, dist2, bad_count)
        with pytest.raises(_lib.OpenSceneAmdError):
            ops.knn_vote(labels, bad_idx, bad_count)


# ---------------------------------------------------------------------------------------------------- blend
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("cols", [3, 768])
def test_k_1_uniform_is_a_bitwise_row_copy(dtype, cols):
    c = case("lattice")
    index = index_of("lattice")
    gen = torch.Generator().manual_seed(cols)
    values = torch.randn((c["xyz"].shape[0], cols), generator=gen).to(dtype)
    values[0, 0], values[1, 1] = -0.0, 6.0e-8                             # a negative zero and (fp16) a subnormal stay as they are
    far = np.full((1, 3), 50.0, dtype=np.float32)                             # a query without a neighbour
    nb = index.knn(torch.from_numpy(np.concatenate([c["queries"], far], 0)).to(dev()), 1)
    out, found = twice(lambda: nb.blend(values.to(dev()), fill=5))
    idx = nb.idx[:, 0].cpu().long()
    assert np.array_equal(found.cpu().numpy(), idx.numpy() >= 0) and found.any() and not found.all()
    assert np.array_equal(bits(out[found]), bits(values[idx[found.cpu()]]))
    assert (out[~found] == 5).all()


@pytest.mark.parametrize("dtype", [np.float16, np.float32])
def test_exact_means_on_the_lattice_are_the_reference_bit_for_bit(dtype):
    c = case("lattice")
    index = index_of("lattice")
    values = c["values"].astype(dtype)
    taken = 0
    for k in (1, 2, 4):
        nb = index.knn(torch.from_numpy(c["queries"]).to(dev()), k, radius=1.0)
        out, found = twice(lambda: nb.blend(torch.from_numpy(values).to(dev())))
        idx, dist, count = ref_knn("lattice", k)
        ref, ref_found = nr.blend(values, idx, dist, count, "uniform", 1.0)
        rows = np.isin(count, (1, 2, 4))                                    # the mean of 1, 2 or 4 multiples of 2^-6 is exact
        taken += int(rows.sum())
        assert np.array_equal(found.cpu().numpy(), ref_found)
        assert np.array_equal(bits(out)[rows], ref[rows].view(bits(out).dtype))
        exact = nr.blend_exact(values, idx, dist, count, "uniform", 1.0)[0]
        assert np.array_equal(ref[rows].astype(np.float64), exact[rows])
    assert taken >= 150


@pytest.mark.parametrize("weights", ["uniform", "inverse"])
@pytest.mark.parametrize("dtype", [np.float16, np.float32])
@pytest.mark.parametrize("cols", [1, 3, 32, 768])
def test_the_blend_stays_within_the_bound_against_float64(cols, dtype, weights):
    c = case("random")
    m = 257 if cols == 768 else 1000
    values = np.random.default_rng(cols).standard_normal((3000, cols)).astype(dtype)
    q, s = torch.from_numpy(c["queries"][:m]).to(dev()), torch.from_numpy(c["qscene"][:m]).to(dev())
    nb = index_of("random").knn(q, 8, scene=s)
    out, found = twice(lambda: nb.blend(torch.from_numpy(values).to(dev()), weights=weights, fill=-3))
    idx, dist, count = (t.cpu().numpy() for t in nb)                        # the kernel's own lists
    exact, absum = nr.blend_exact(values, idx, dist, count, weights, c["voxel_size"])
    bound = nr.blend_bound(exact, absum, count, dtype)
    out, found = out.cpu().numpy(), found.cpu().numpy()
    assert np.array_equal(found, count > 0) and found.any() and not found.all()
    assert (out[~found] == -3).all()                                        # count == 0 gives fill
    err = np.abs(out.astype(np.float64) - exact)[found]
    print("blend C=%d %s %s: max err / bound = %.3f" % (cols, np.dtype(dtype).name, weights, float((err / bound[found]).max())))
    assert (err <= bound[found]).all()


# ---------------------------------------------------------------------------------------------------- vote
@pytest.mark.parametrize("k", [1, 4, 16])
def test_the_vote_is_the_reference(k):
    c = case("lattice")
    nb = index_of("lattice").knn(torch.from_numpy(c["queries"]).to(dev()), k, radius=1.0)
    idx, _dist, count = ref_knn("lattice", k)
    for labels in (c["labels"], np.full_like(c["labels"], -1), np.arange(c["labels"].shape[0], dtype=np.int64) % 2 + (1 << 40)):
        got, = twice(lambda: (nb.vote(torch.from_numpy(labels).to(dev()), fill=-7),))
        ref = nr.vote(labels, idx, count, fill=-7)
        assert np.array_equal(got.cpu().numpy(), ref)
    ref = nr.vote(c["labels"], idx, count, fill=-7)
    assert (ref == -7).any() and (ref >= 0).any()                          # no labelled neighbour, and winners


# ---------------------------------------------------------------------------------------------------- end to end
def test_fill_missing_mends_the_object_and_transfer_to_the_own_points_is_the_identity():
    from openscene_amd import neighbors as N
    from openscene_amd.objects import find_objects
    c = case("room")
    grid = index_of("room").grid
    heat, holed, seen = (torch.from_numpy(c[key]).to(dev()) for key in ("heat", "holed", "seen"))
    filled, missing = twice(lambda: N.fill_missing(grid, holed, seen, k=4))
    unseen = ~c["seen"]
    idx, dist, count = nr.knn(c["xyz"], c["offsets"], 0.05, c["xyz"][unseen], 0, 4, sources=c["seen"])
    ref, found = nr.blend(c["holed"], idx, dist, count, "inverse", 0.05)
    assert np.array_equal(bits(filled[seen]), bits(holed[seen]))
    assert np.array_equal(bits(filled)[unseen], ref.view(np.uint16))
    assert np.array_equal(missing.cpu().numpy()[unseen], ~found) and not missing.cpu().numpy()[c["seen"]].any()
    assert int(find_objects(grid, holed, c["threshold"]).n_objects[0, 0]) >= 2
    assert int(find_objects(grid, filled, c["threshold"]).n_objects[0, 0]) == 1
    out, found = twice(lambda: N.transfer(index_of("room"), grid.xyz, heat, k=1))
    assert bool(found.all()) and np.array_equal(bits(out), bits(heat))
    wide = torch.randn((grid.n_points, 768), generator=torch.Generator().manual_seed(0)).half().to(dev())      # an fp16 feature matrix
    filled, _ = N.fill_missing(grid, wide, seen, k=4)
    assert np.array_equal(bits(filled[seen]), bits(wide[seen])) and bool(torch.isfinite(filled).all())
