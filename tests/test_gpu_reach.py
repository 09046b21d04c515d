"""csrc/reach.hip and what is built on it on the device against the numpy restatement of tests/reach_reference.py: the search
bit for bit (dist2 and nearest), the second stage of knn / knn_self / transfer / fill_missing bit for bit in idx, the bits of
dist2 and count, the blend of the filled rows within neighbors_reference.blend_bound.  Every shape is small: at most 3 000
cells."""
import functools
import itertools

import numpy as np
import pytest
import torch

import neighbors_reference as nr
import reach_reference as rr

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda", 0)


def on(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def search(q, src, ids, reach):
    """ops.reach_nearest, twice (the two results equal bit for bit) -> (nearest, dist2) as numpy."""
    from openscene_amd import ops
    a = ops.reach_nearest(on(q), on(src), on(ids), reach)
    b = ops.reach_nearest(on(q), on(src), on(ids), reach)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert a[0].dtype == torch.int32 and a[1].dtype == torch.int32
    return a[0].cpu().numpy(), a[1].cpu().numpy()


def check(q, src, ids, reach):
    got = search(q, src, ids, reach)
    ref = rr.nearest(q, src, ids, reach)
    assert np.array_equal(got[1], ref[1]) and np.array_equal(got[0], ref[0])
    return got


def one(query, sources, reach, ids=None):
    src = rr.rows(0, sources)
    ids = np.arange(src.shape[0], dtype=np.int32) if ids is None else np.asarray(ids, dtype=np.int32)
    near, d2 = check(rr.rows(0, [query]), src, ids, reach)
    return int(near[0]), int(d2[0])


@functools.lru_cache(maxsize=None)
def grid_of(name):
    from openscene_amd.objects import VoxelGrid
    c = getattr(rr if name in ("hole", "icp", "near") else nr, name + "_case")()
    xyz = c["b"] if name == "icp" else c["xyz"]
    return VoxelGrid(on(xyz), c.get("offsets", [0, xyz.shape[0]]), voxel_size=c["voxel_size"])


def bits(t):
    a = t.cpu().numpy()
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same(got, ref):
    idx, dist, count = ref
    assert np.array_equal(got.count.cpu().numpy(), count)
    assert np.array_equal(got.idx.cpu().numpy(), idx)
    assert np.array_equal(bits(got.dist2), dist.view(np.uint32))


# ---------------------------------------------------------------------------------------------------- the search
@pytest.mark.parametrize("c,s", [(0, 3000), (1, 1), (255, 511), (256, 512), (257, 513), (1000, 3000), (1000, 0), (1, 3000), (257, 1)])
def test_the_random_case_bit_for_bit(c, s):
    q, src, ids = rr.random_case(c, s)
    for reach in rr.REACHES:
        check(q, src, ids, reach)


@pytest.mark.parametrize("c", rr.RANDOM_C)
@pytest.mark.parametrize("s", rr.RANDOM_S)
def test_every_pair_of_sizes_at_two_reaches(c, s):
    q, src, ids = rr.random_case(c, s, seed=1)
    check(q, src, ids, 8)
    check(q, src, ids, 4096)


def test_a_ball_not_a_cube():
    assert one((0, 0, 0), [(2, 2, 1)], 3) == (0, 9)
    assert one((0, 0, 0), [(2, 2, 2)], 3) == (-1, -1)
    assert one((0, 0, 0), [(2, 2, 2), (-3, 0, 0)], 3) == (1, 9)
    for axis, sign in itertools.product(range(3), (-1, 1)):
        at = [1, 2, 3]
        at[axis] += 5 * sign
        assert one((1, 2, 3), [tuple(at)], 5) == (0, 25)                     # exactly `reach` along one axis
        assert one((1, 2, 3), [tuple(at)], 4) == (-1, -1)                    # reach + 1
    assert one((4, 4, 4), [(4, 4, 4)], 1) == (0, 0)


def test_ties_go_to_the_lowest_id_whatever_the_order_of_the_sources():
    ring = [(3, 0, 0), (-3, 0, 0), (0, 3, 0), (0, 0, -3), (2, 2, 1), (1, -2, 2), (-2, 1, -2)]          # all d2 = 9
    base = np.array([4, 9, 2, 7, 3, 8, 5])
    for perm in (np.arange(7), np.arange(7)[::-1], np.random.default_rng(0).permutation(7)):
        assert one((0, 0, 0), [ring[i] for i in perm], 3, base[perm]) == (2, 9)
    for k in (1, 5, 8, 9):                                                   # +-k on one axis, across block faces
        assert one((0, 0, 0), [(k, 0, 0), (-k, 0, 0)], 9, [7, 3]) == (3, k * k)
        assert one((0, 0, 0), [(0, -k, 0), (0, k, 0)], 9, [7, 3]) == (3, k * k)


def test_the_integer_range():
    assert one((-20000, 0, 0), [(26341, 0, 0)], 4096) == (-1, -1)            # dx = 46 341: its square is above 2^31
    assert one((-32766, 0, 0), [(32766, 0, 0)], 4096) == (-1, -1)            # dx = 65 532: its square wraps negative in 32 bits
    assert one((32766, -32766, 7), [(-32766, 32766, 7)], 4096) == (-1, -1)
    assert one((-32766, 5, 5), [(-32766 + 4096, 5, 5)], 4096) == (0, 4096 * 4096)
    assert one((-20000, 0, 0), [(-20000 + 4096, 0, 0)], 4096) == (0, 4096 * 4096)
    assert one((32766, 32766, 32766), [(32766 - 2000, 32766 - 2000, 32766 - 2000)], 4096) == (0, 3 * 2000 * 2000)
    assert one((-32766, -32766, -32766), [(-32766, -32766, -32766 + 1)], 1) == (0, 1)


def test_block_edges_a_far_block_and_a_full_block():
    q, src, ids = rr.block_edge_case()
    for reach in (1, 7, 8, 9, 17):
        check(q, src, ids, reach)
    q, src, ids = rr.far_block_case()
    assert [x.tolist() for x in check(q, src, ids, 16)] == [[1], [81]]
    q, src, ids = rr.full_block_case()
    near, d2 = check(q, src, ids, 6)
    assert d2.tolist() == [0, 0, 1, 16, 27, 0, 3, -1]
    check(q, src, ids, 4096)
    twice = np.concatenate([src, src[:300]], 0)                              # repeated cells: a block of more than 512 entries
    check(q, twice, np.random.default_rng(5).permutation(813).astype(np.int32), 6)


def test_scenes_never_mix():
    q = np.array([[0, 0, 0, 0], [1, 0, 0, 0], [2, 0, 0, 0]], dtype=np.int32)
    src = np.array([[1, 1, 0, 0], [0, 5, 0, 0], [3, 0, 0, 0]], dtype=np.int32)
    near, d2 = check(q, src, np.array([0, 1, 2], dtype=np.int32), 8)
    assert near.tolist() == [1, 0, -1] and d2.tolist() == [25, 1, -1]


def test_permuting_the_sources_changes_nothing():
    q, src, ids = rr.random_case(1000, 3000)
    perm = np.random.default_rng(9).permutation(3000)
    for reach in (2, 9):
        a = search(q, src, ids, reach)
        b = search(q, src[perm], ids[perm], reach)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---------------------------------------------------------------------------------------------------- on a grid
def test_reach_one_is_the_minimum_over_the_grids_own_table():
    from openscene_amd import reach as R
    c = nr.random_case()
    grid = grid_of("random")
    sources = np.random.default_rng(2).random(3000) < 0.03
    f = R.distance_field(grid, on(sources), 1)
    nbr, inverse = grid.nbr.cpu().numpy(), grid.inverse.cpu().numpy()
    held = rr.source_voxels(inverse, nbr.shape[1], sources)
    offs = nr.OFFSETS                                                        # the 27 offsets of the table, in its order
    want_d2, want = np.full(nbr.shape[1], -1), np.full(nbr.shape[1], -1)
    for v in range(nbr.shape[1]):
        keys = [(sum(abs(x) for x in offs[o]), nbr[o, v]) for o in range(27) if sum(abs(x) for x in offs[o]) <= 1 and nbr[o, v] >= 0 and held[nbr[o, v]]]
        if keys:
            want_d2[v], want[v] = min(keys)
    assert np.array_equal(f.dist2.cpu().numpy(), want_d2) and np.array_equal(f.nearest.cpu().numpy(), want)
    assert (want_d2 == 1).sum() >= 20 and (want_d2 == -1).sum() >= 20
    d2, near = rr.field(c["xyz"], c["offsets"], c["voxel_size"], sources, 1)
    assert np.array_equal(want_d2, d2) and np.array_equal(want, near)


def test_distance_field_nearest_voxel_and_near():
    from openscene_amd import reach as R
    from openscene_amd.objects import find_objects
    c = rr.near_case()
    grid = grid_of("near")
    coords, inverse = rr.voxels(c["xyz"], c["offsets"], 0.05)
    assert np.array_equal(grid.coords.cpu().numpy(), coords)
    sources = np.random.default_rng(0).random(1200) < 0.02
    f = R.distance_field(grid, on(sources), 30)
    d2, near = rr.field(c["xyz"], c["offsets"], 0.05, sources, 30)
    assert np.array_equal(f.dist2.cpu().numpy(), d2) and np.array_equal(f.nearest.cpu().numpy(), near)
    assert np.array_equal(f.within(0.12).cpu().numpy(), rr.within(d2, inverse, 0.12, 0.05))
    q = np.random.default_rng(1).uniform(-0.3, 1.3, (200, 3)).astype(np.float32)
    q[3, 0] = np.nan
    scene = np.random.default_rng(1).integers(0, 2, 200)
    got = R.nearest_voxel(grid, on(q), on(scene), on(sources), 6)
    ok, cell = nr.query_valid(q, scene, 2, 0.05)
    held = rr.source_voxels(inverse, coords.shape[0], sources)
    ref = rr.nearest(np.concatenate([scene[:, None], np.where(ok[:, None], cell, 0).astype(np.int64)], 1)[ok], coords[held], np.nonzero(held)[0], 6)
    assert np.array_equal(got[0].cpu().numpy()[ok], ref[0]) and np.array_equal(got[1].cpu().numpy()[ok], ref[1]) and int(got[0][3]) == -1
    out = R.near(grid, on(c["heat"]), 0, 1, 0.5, c["distance"])
    assert np.array_equal(bits(out), rr.near(c["xyz"], c["offsets"], 0.05, c["heat"], 0, 1, 0.5, c["distance"]).view(np.uint16))
    assert int(find_objects(grid, out, 0.5).n_objects.sum()) >= 1


# ---------------------------------------------------------------------------------------------------- the second stage
@pytest.mark.parametrize("name", ["lattice", "crowded", "two_scene", "empty", "random"])
def test_knn_without_reach_is_what_it_was_and_with_reach_the_restatement(name):
    from openscene_amd.neighbors import PointIndex
    c = getattr(nr, name + "_case")()
    index = PointIndex(grid_of(name))
    queries, qscene = c["queries"][:300], c["qscene"][:300]
    q, s = on(queries), on(qscene)
    same(index.knn(q, 5, radius=c["radius"], scene=s), nr.knn(c["xyz"], c["offsets"], c["voxel_size"], queries, qscene, 5, c["radius"]))
    for k, reach, radius in ((1, 3, None), (5, 40, c["radius"])):
        ref = rr.knn(c["xyz"], c["offsets"], c["voxel_size"], queries, qscene, k, reach, radius)
        same(index.knn(q, k, radius=radius, scene=s, reach=reach), ref)
        first = nr.knn(c["xyz"], c["offsets"], c["voxel_size"], queries, qscene, k, rr.radius_of(c["voxel_size"], reach, radius))
        kept = first[2] > 0
        assert np.array_equal(ref[0][kept], first[0][kept]) and np.array_equal(ref[1][kept].view(np.uint32), first[1][kept].view(np.uint32))


def test_knn_self_transfer_and_the_hole():
    from openscene_amd import neighbors as N
    c = rr.hole_case()
    grid = grid_of("hole")
    n = c["xyz"].shape[0]
    scene = np.zeros(n, dtype=np.int64)
    seen, holed = on(c["seen"]), on(c["holed"])
    index = N.PointIndex(grid, seen)
    same(index.knn_self(4), nr.knn(c["xyz"], c["offsets"], 0.05, c["xyz"], scene, 4, 0.05, sources=c["seen"]))
    same(index.knn_self(4, reach=3), rr.knn(c["xyz"], c["offsets"], 0.05, c["xyz"], scene, 4, 3, sources=c["seen"]))
    same(index.knn_self(2, radius=0.12, include_self=False, reach=2),
         rr.knn(c["xyz"], c["offsets"], 0.05, c["xyz"], scene, 2, 2, 0.12, sources=c["seen"], exclude=np.arange(n, dtype=np.int32)))
    q = (c["xyz"][::7] + np.float32(0.2) * np.array([0, 0, 1], dtype=np.float32)).astype(np.float32)
    out, found = N.transfer(index, on(q), on(c["values"]), k=1, reach=6)
    idx, dist, count = rr.knn(c["xyz"], c["offsets"], 0.05, q, 0, 1, 6, sources=c["seen"])
    assert found.all() and np.array_equal(bits(out), c["values"][idx[:, 0]].view(np.uint16))          # k = 1 uniform: a copy of the row
    assert not N.transfer(index, on(q), on(c["values"]), k=1)[1].any()
    # the hole
    before, missing_before = N.fill_missing(grid, holed, seen, k=c["k"])
    filled, missing = N.fill_missing(grid, holed, seen, k=c["k"], reach=c["reach"])
    first, both = rr.fill_lists(c["xyz"], c["offsets"], 0.05, c["seen"], c["k"], c["reach"])
    unseen = ~c["seen"]
    assert np.array_equal(missing_before.cpu().numpy(), unseen & (first[2] == 0)) and int(missing_before.sum()) >= 50
    assert not missing.any()
    assert np.array_equal(bits(filled)[c["seen"]], c["holed"][c["seen"]].view(np.uint16))
    was = (~missing_before).cpu().numpy()
    assert np.array_equal(bits(filled)[was], bits(before)[was])
    exact, absum = nr.blend_exact(c["holed"], both[0], both[1], both[2], "inverse", 0.05)
    bound = nr.blend_bound(exact, absum, both[2], np.float16)
    err = np.abs(filled.cpu().numpy().astype(np.float64) - exact)[unseen]
    assert (err <= bound[unseen]).all(), float((err / bound[unseen]).max())


def test_icp_with_reach_pairs_the_displaced_plane():
    from openscene_amd.align import RigidTransform, refine_icp
    from openscene_amd.neighbors import PointIndex
    c = rr.icp_case()
    index = PointIndex(grid_of("icp"))
    a = on(c["a"])
    fit = refine_icp(index, a, RigidTransform(), iterations=10)
    assert not fit.ok and fit.count < 3 and bool((fit.neighbors == -1).all())
    first = refine_icp(index, a, RigidTransform(), iterations=0, reach=c["reach"])
    assert np.array_equal(first.neighbors.cpu().numpy(), rr.knn(c["b"], [0, 800], 0.05, c["a"], 0, 1, c["reach"])[0][:, 0]) and first.count == 800
    fit = refine_icp(index, a, RigidTransform(), iterations=10, reach=c["reach"])
    offset = float(np.abs(fit.transform.apply(c["a"])[:, 2].mean() - c["b"][:, 2].astype(np.float64).mean()))
    print("normal offset after ICP with reach: %.3g voxel sizes" % (offset / 0.05))
    assert fit.ok and fit.count == 800 and offset < 0.05


# ---------------------------------------------------------------------------------------------------- argument errors
def test_bad_arguments_on_the_device():
    from openscene_amd import ops
    from openscene_amd import reach as R
    from openscene_amd._lib import OpenSceneAmdError
    from openscene_amd.neighbors import PointIndex
    q, src, ids = rr.random_case(257, 513)
    for reach in (0, 4097):
        with pytest.raises(ValueError):
            ops.reach_nearest(on(q), on(src), on(ids), reach)
    with pytest.raises(TypeError):
        ops.reach_nearest(on(q).long(), on(src), on(ids), 4)
    with pytest.raises(ValueError):
        ops.reach_nearest(on(q)[:, :3], on(src), on(ids), 4)
    with pytest.raises(ValueError):
        ops.reach_nearest(on(q), on(src), on(ids)[:5], 4)
    with pytest.raises(ValueError):
        ops.reach_nearest(on(q), torch.from_numpy(src), on(ids), 4)          # sources on another device
    far = q.copy()
    far[3, 2] = 40000                                                        # a cell outside the packable range: skipped and reported
    with pytest.raises(OpenSceneAmdError):
        ops.reach_nearest(on(far), on(src), on(ids), 4)
    grid = grid_of("near")
    index = PointIndex(grid)
    with pytest.raises(ValueError):
        index.knn(torch.zeros((4, 3), device=dev()), 1, radius=0.1501, reach=2)                       # (reach + 1) * voxel_size = 0.15
    with pytest.raises(ValueError):
        R.distance_field(grid, torch.zeros(1199, dtype=torch.bool, device=dev()), 2)
    with pytest.raises(ValueError):
        R.distance_field(grid, torch.zeros(1200, dtype=torch.bool), 2)       # a mask on the host
