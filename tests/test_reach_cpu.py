"""Host logic of openscene_amd.reach and of the second stage `reach=` of openscene_amd.neighbors WITHOUT a GPU: ops.reach_nearest
is replaced by the stand-in of tests/reach_reference.py (the kernel's contract in numpy), the neighbour ops by those of
tests/neighbors_reference.py and the grid's ops by those of tests/objects_reference.py, so distance_field, nearest_voxel, near,
PointIndex._stage2, transfer, fill_missing and refine_icp are the code under test; the wrapper's argument checks and its plan
(the sort by 8^3 block, the work items) run as they are.  The restatement's own invariants -- what tests/test_gpu_reach.py relies
on -- are checked here, on the same inputs."""
import os
import re

import numpy as np
import pytest
import torch

import align_reference as ar
import neighbors_reference as nr
import objects_reference as oref
import reach_reference as rr
from openscene_amd import _lib
from openscene_amd import align
from openscene_amd import neighbors as N
from openscene_amd import ops
from openscene_amd import reach as R
from openscene_amd.objects import VoxelGrid, find_objects

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REAL_REACH = ops.reach_nearest


@pytest.fixture(autouse=True)
def cpu_kernels(monkeypatch):
    for name, f in (("coords_unique", oref.coords_unique), ("kmap_build", oref.kmap_build), ("objects_find", oref.objects_find),
                    ("knn_grid", nr.knn_grid), ("knn_blend", nr.knn_blend), ("knn_vote", nr.knn_vote), ("reach_nearest", rr.reach_nearest)):
        monkeypatch.setattr(ops, name, f)


def grid_of(xyz, offsets, voxel_size):
    return VoxelGrid(torch.from_numpy(xyz), offsets, voxel_size=voxel_size)


def same(got, ref):
    idx, dist, count = ref
    assert np.array_equal(got.count.numpy(), count)
    assert np.array_equal(got.idx.numpy(), idx)
    assert np.array_equal(got.dist2.numpy().view(np.uint32), dist.view(np.uint32))


def one(query, sources, reach, ids=None):
    """The restatement for one query cell of scene 0 -> (nearest, dist2)."""
    src = rr.rows(0, sources)
    near, d2 = rr.nearest(rr.rows(0, [query]), src, np.arange(src.shape[0]) if ids is None else ids, reach)
    return int(near[0]), int(d2[0])


# ---------------------------------------------------------------------------------------------------- registration
def test_the_header_the_prototype_and_the_build_name_the_entry():
    src = open(os.path.join(ROOT, "include", "openscene_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = {n for n in re.findall(r"\b(osn_[a-z0-9_]+)\s*\(", code) if n.startswith("osn_reach_")}
    assert declared == {"osn_reach_nearest"} == {n for n in _lib.PROTOTYPES if n.startswith("osn_reach_")}
    decl = re.search(r"osn_reach_nearest\s*\((.*?)\);", code, flags=re.S).group(1)
    assert len(decl.split(",")) == len(_lib.PROTOTYPES["osn_reach_nearest"][1])
    assert src.index("csrc/neighbors.hip") < src.index("int osn_knn_vote(") < src.index("csrc/reach.hip") < src.index("int osn_reach_nearest(")
    block = src[src.index("csrc/reach.hip"):src.index("int osn_reach_nearest(")]
    for word in ("uint32(d2) << 32 | uint32(id)", "d2 <= reach^2", "lowest id", "|c| < 32767", "before any square", "cell >> 3", "-1 without a candidate"):
        assert word in block, word
    from openscene_amd import build
    assert "reach.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "reach.hip"))


# ---------------------------------------------------------------------------------------------------- the restatement itself
def test_a_ball_not_a_cube():
    assert one((0, 0, 0), [(2, 2, 1)], 3) == (0, 9)
    assert one((0, 0, 0), [(2, 2, 2)], 3) == (-1, -1)                        # d2 = 12 > 9, inside the cube
    assert one((0, 0, 0), [(2, 2, 2), (-3, 0, 0)], 3) == (1, 9)
    for axis in range(3):
        for sign in (-1, 1):
            at = [0, 0, 0]
            at[axis] = 5 * sign
            assert one((1, 2, 3), [(1 + at[0], 2 + at[1], 3 + at[2])], 5) == (0, 25)
            assert one((1, 2, 3), [(1 + at[0], 2 + at[1], 3 + at[2])], 4) == (-1, -1)
    assert one((4, 4, 4), [(4, 4, 4)], 1) == (0, 0)                          # a query that is itself a source


def test_ties_go_to_the_lowest_id_and_the_range_is_exact():
    ring = [(3, 0, 0), (-3, 0, 0), (0, 3, 0), (0, 0, -3), (2, 2, 1), (1, -2, 2), (-2, 1, -2)]          # all d2 = 9
    for perm in (np.arange(7), np.arange(7)[::-1], np.random.default_rng(0).permutation(7)):
        ids = np.array([4, 9, 2, 7, 3, 8, 5])[perm]
        assert one((0, 0, 0), [ring[i] for i in perm], 3, ids) == (2, 9)
    assert one((-20000, 0, 0), [(26341, 0, 0)], 4096) == (-1, -1)            # dx = 46 341: its square is above 2^31
    assert one((-32766, 0, 0), [(32766, 0, 0)], 4096) == (-1, -1)            # dx = 65 532: its square wraps negative in 32 bits
    assert one((-32766, 5, 5), [(-32766 + 4096, 5, 5)], 4096) == (0, 4096 * 4096)
    assert one((32766, 32766, 32766), [(32766 - 2000, 32766 - 2000, 32766 - 2000)], 4096) == (0, 3 * 2000 * 2000)
    assert 46341 ** 2 > 2 ** 31 and np.array(65532 ** 2 & 0xFFFFFFFF, dtype=np.uint32).view(np.int32) < 0


def test_the_cases_hold_what_the_gpu_tests_rely_on():
    q, src, ids = rr.random_case(1000, 3000)
    near, d2 = rr.nearest(q, src, ids, 8)
    assert sorted(ids.tolist()) == list(range(3000)) and not np.array_equal(ids, np.arange(3000))
    assert set(q[:, 0]) == {0, 1} and set(src[:, 0]) == {0, 2}              # scene 1: no sources; scene 2: no queries
    assert (near[q[:, 0] == 1] == -1).all() and (near[q[:, 0] == 0] >= 0).all() and (d2[q[:, 0] == 0] == 0).any()
    where = {int(i): s for i, s in zip(ids, src[:, 0])}
    assert all(where[int(n)] == 0 for n in near if n >= 0)                   # never a source of another scene
    near1, _ = rr.nearest(q, src, ids, 1)
    assert ((near1 == -1) & (q[:, 0] == 0)).any() and (near1 >= 0).any()     # reach 1 loses some, not all
    # block edges: nearest sources across block faces; the far block beats the adjacent one; the full block and its neighbour
    q, src, ids = rr.block_edge_case()
    near, d2 = rr.nearest(q, src, ids, 9)
    cell_of = {int(i): s[1:] for i, s in zip(ids, src)}
    crossing = sum(1 for c, n in zip(q, near) if n >= 0 and ((c[1:] >> 3) != (cell_of[int(n)] >> 3)).any())
    assert (near >= 0).all() and crossing >= 20 and (d2 == 0).sum() == src.shape[0]
    q, src, ids = rr.far_block_case()
    assert rr.nearest(q, src, ids, 16)[0].tolist() == [1] and rr.nearest(q, src, ids, 16)[1].tolist() == [81]
    q, src, ids = rr.full_block_case()
    near, d2 = rr.nearest(q, src, ids, 6)
    assert src.shape[0] == 513 and len({tuple(r >> 3) for r in src[:512, 1:]}) == 1 and tuple(src[512, 1:] >> 3) == (1, 0, 0)
    assert d2.tolist() == [0, 0, 1, 16, 27, 0, 3, -1] and near[1] == ids[512] and near[2] == ids[512] and near[7] == -1
    # the hole: 5 voxels wide, the 27 cells do not close it, reach 8 does
    c = rr.hole_case()
    cells = np.floor(c["xyz"].astype(np.float64) / 0.05).astype(np.int64)
    assert sorted(set(cells[~c["seen"], 0])) == [8, 9, 10, 11, 12] and set(cells[:, 2]) == {0}
    first, both = rr.fill_lists(c["xyz"], c["offsets"], 0.05, c["seen"], c["k"], c["reach"])
    unseen = ~c["seen"]
    assert (first[2][unseen] == 0).sum() >= 50 and (first[2][unseen] > 0).sum() >= 50 and (both[2][unseen] > 0).all()
    kept = first[2] > 0
    assert np.array_equal(both[0][kept], first[0][kept]) and np.array_equal(both[1][kept].view(np.uint32), first[1][kept].view(np.uint32))
    # ICP: the first round of the 27 cells pairs nothing; with reach 4 every point is paired, many with their own twin
    c = rr.icp_case()
    assert (nr.knn(c["b"], [0, 800], 0.05, c["a"], 0, 1, 0.05)[2] == 0).all()
    idx, _, count = rr.knn(c["b"], [0, 800], 0.05, c["a"], 0, 1, c["reach"])
    assert (count == 1).all() and (idx[:, 0] == np.arange(800)).sum() >= 200 and (idx[:, 0] != np.arange(800)).sum() >= 200
    # near: both scenes keep some and drop some; scene 1's anchor lies left of x = 0.3
    c = rr.near_case()
    out = rr.near(c["xyz"], c["offsets"], 0.05, c["heat"], 0, 1, 0.5, c["distance"])
    for s in (0, 1):
        part = out[c["offsets"][s]:c["offsets"][s + 1], 0]
        assert np.isfinite(part).sum() >= 30 and np.isneginf(part).sum() >= 300


# ---------------------------------------------------------------------------------------------------- the plan (torch, as it runs)
@pytest.mark.parametrize("c,s", [(1, 1), (257, 513), (1000, 3000)])
def test_the_plan_sorts_by_block_and_cuts_items_at_scene_boundaries(c, s):
    q, src, ids = rr.random_case(c, s)
    qs, order, items, packed, blocks, start = (t.numpy() for t in ops.reach_plan(torch.from_numpy(q), torch.from_numpy(src), torch.from_numpy(ids)))
    assert np.array_equal(qs, q[order]) and sorted(order.tolist()) == list(range(c))
    by_id = {int(i): r for i, r in zip(ids, src)}
    assert start[0] == 0 and start[-1] == s and (np.diff(start) > 0).all() and len({tuple(b) for b in blocks}) == blocks.shape[0]
    for b in range(blocks.shape[0]):
        for x, y, z, i in packed[start[b]:start[b + 1]]:
            assert tuple(by_id[int(i)]) == (blocks[b, 0], x, y, z) and (x >> 3, y >> 3, z >> 3) == tuple(blocks[b, 1:])
    covered = []
    for a, e, b0, b1 in items:
        assert 0 < e - a <= ops.REACH_ITEM and len(set(qs[a:e, 0])) == 1
        assert np.array_equal(np.nonzero(blocks[:, 0] == qs[a, 0])[0], np.arange(b0, b1))
        covered += list(range(a, e))
    assert covered == list(range(c))
    keys = [tuple(r) for r in np.concatenate([qs[:, :1], qs[:, 1:] >> 3], 1)]
    assert keys == sorted(keys)


# ---------------------------------------------------------------------------------------------------- the distance field
def test_distance_field_nearest_voxel_and_near_are_the_restatement():
    c = rr.near_case()
    grid = grid_of(c["xyz"], c["offsets"], 0.05)
    coords, inverse = rr.voxels(c["xyz"], c["offsets"], 0.05)
    assert np.array_equal(grid.coords.numpy(), coords) and np.array_equal(grid.inverse.numpy(), inverse)
    sources = np.random.default_rng(0).random(1200) < 0.02
    for reach in (1, 3, 30):
        f = R.distance_field(grid, torch.from_numpy(sources), reach)
        d2, near = rr.field(c["xyz"], c["offsets"], 0.05, sources, reach)
        assert np.array_equal(f.dist2.numpy(), d2) and np.array_equal(f.nearest.numpy(), near) and f.dist2.dtype == torch.int32
        dist = np.where(d2 >= 0, np.sqrt(np.maximum(d2, 0).astype(np.float32)) * np.float32(0.05), np.float32(np.inf)).astype(np.float32)
        assert np.array_equal(f.distance().numpy().view(np.uint32), dist.view(np.uint32))
        assert np.array_equal(f.at_points().numpy().view(np.uint32), dist[inverse].view(np.uint32))
        for distance in (0.0, 0.05, 0.1, 0.12, 2.0):
            assert np.array_equal(f.within(distance).numpy(), rr.within(d2, inverse, distance, 0.05))
    held = rr.source_voxels(inverse, coords.shape[0], sources)
    f = R.distance_field(grid, torch.from_numpy(held), 3, per_voxel=True)
    assert np.array_equal(f.dist2.numpy(), rr.field(c["xyz"], c["offsets"], 0.05, sources, 3)[0])
    assert (f.dist2.numpy()[held] == 0).all() and np.array_equal(f.nearest.numpy()[held], np.nonzero(held)[0])
    # foreign positions, some invalid
    rng = np.random.default_rng(1)
    q = rng.uniform(-0.3, 1.3, (200, 3)).astype(np.float32)
    q[3, 0], q[4, 1], q[5, 2] = np.nan, np.inf, 1e9
    scene = rng.integers(0, 2, 200)
    scene[6], scene[7] = 2, -1
    near, d2 = R.nearest_voxel(grid, torch.from_numpy(q), torch.from_numpy(scene), torch.from_numpy(sources), 6)
    ok, cell = nr.query_valid(q, scene, 2, 0.05)
    cells = np.concatenate([scene[:, None], np.where(ok[:, None], cell, 0).astype(np.int64)], 1)
    ref = rr.nearest(cells[ok], coords[held], np.nonzero(held)[0], 6)
    assert not ok[3:8].any() and (near.numpy()[~ok] == -1).all() and (d2.numpy()[~ok] == -1).all()
    assert np.array_equal(near.numpy()[ok], ref[0]) and np.array_equal(d2.numpy()[ok], ref[1]) and (ref[0] >= 0).any() and (ref[0] < 0).any()
    # near, and what takes it
    heat = torch.from_numpy(c["heat"])
    out = R.near(grid, heat, 0, 1, 0.5, c["distance"])
    assert out.dtype == torch.float16 and tuple(out.shape) == (1200, 1)
    assert np.array_equal(out.numpy().view(np.uint16), rr.near(c["xyz"], c["offsets"], 0.05, c["heat"], 0, 1, 0.5, c["distance"]).view(np.uint16))
    assert int(find_objects(grid, out, 0.5).n_objects.sum()) >= 1
    from openscene_amd.search import SearchResult
    res = SearchResult(["a", "b"], c["offsets"], None, None, None, heat)
    assert torch.equal(res.near(grid, 0, 1, 0.5, c["distance"]).view(torch.int16), out.view(torch.int16))


# ---------------------------------------------------------------------------------------------------- the second stage
def test_without_reach_the_new_op_is_never_called(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("ops.reach_nearest on the reach=None path")
    monkeypatch.setattr(ops, "reach_nearest", refuse)
    c = nr.empty_case()
    grid = grid_of(c["xyz"], c["offsets"], c["voxel_size"])
    index = N.PointIndex(grid)
    q, s = torch.from_numpy(c["queries"]), torch.from_numpy(c["qscene"])
    same(index.knn(q, 4, radius=c["radius"], scene=s), nr.knn(c["xyz"], c["offsets"], c["voxel_size"], c["queries"], c["qscene"], 4, c["radius"]))
    index.knn_self(4)
    values = torch.zeros((100, 2))
    N.transfer(index, q, values, scene=s)
    N.fill_missing(grid, values, torch.arange(100) % 3 > 0)
    with pytest.raises(AssertionError):
        index.knn(q, 4, scene=s, reach=2)


@pytest.mark.parametrize("name", ["lattice", "crowded", "two_scene", "empty", "random"])
def test_knn_with_reach_is_the_restatement_and_keeps_the_first_stage(name):
    c = getattr(nr, name + "_case")()
    queries, qscene = c["queries"][:200], c["qscene"][:200]
    grid = grid_of(c["xyz"], c["offsets"], c["voxel_size"])
    index = N.PointIndex(grid)
    q, s = torch.from_numpy(queries), torch.from_numpy(qscene)
    for k, reach, radius in ((1, 3, None), (5, 40, c["radius"]), (4, 2, 2.5 * c["voxel_size"])):
        got = index.knn(q, k, radius=radius, scene=s, reach=reach)
        ref = rr.knn(c["xyz"], c["offsets"], c["voxel_size"], queries, qscene, k, reach, radius)
        same(got, ref)
        first = nr.knn(c["xyz"], c["offsets"], c["voxel_size"], queries, qscene, k, rr.radius_of(c["voxel_size"], reach, radius))
        kept = first[2] > 0
        assert np.array_equal(ref[0][kept], first[0][kept]) and np.array_equal(ref[2][kept], first[2][kept])
    if name == "empty":                                                      # the far queries now find the cloud; the invalid ones never
        count = index.knn(q, 2, scene=s, reach=200).count.tolist()
        assert count[:2] == [2, 2] and count[2:8] == [0] * 6


def test_knn_self_exclude_sources_and_transfer_with_reach():
    c = rr.hole_case()
    grid = grid_of(c["xyz"], c["offsets"], 0.05)
    n = c["xyz"].shape[0]
    scene = np.zeros(n, dtype=np.int64)
    own = np.arange(n, dtype=np.int32)
    index = N.PointIndex(grid, torch.from_numpy(c["seen"]))
    same(index.knn_self(4, reach=3), rr.knn(c["xyz"], c["offsets"], 0.05, c["xyz"], scene, 4, 3, sources=c["seen"]))
    same(index.knn_self(2, radius=0.12, include_self=False, reach=2),
         rr.knn(c["xyz"], c["offsets"], 0.05, c["xyz"], scene, 2, 2, 0.12, sources=c["seen"], exclude=own))
    q = (c["xyz"][::7] + np.float32(0.2) * np.array([0, 0, 1], dtype=np.float32)).astype(np.float32)
    values = torch.from_numpy(c["values"])
    out, found = N.transfer(index, torch.from_numpy(q), values, k=3, weights="inverse", reach=6)
    idx, dist, count = rr.knn(c["xyz"], c["offsets"], 0.05, q, 0, 3, 6, sources=c["seen"])
    ref, ref_found = nr.blend(c["values"], idx, dist, count, "inverse", 0.05)
    assert found.all() and np.array_equal(found.numpy(), ref_found) and np.array_equal(out.numpy().view(np.uint16), ref.view(np.uint16))
    assert not N.transfer(index, torch.from_numpy(q), values, k=3)[1].any()  # four cells up: nothing without reach


def test_fill_missing_with_reach_closes_the_hole_and_keeps_what_it_filled_before():
    c = rr.hole_case()
    grid = grid_of(c["xyz"], c["offsets"], 0.05)
    holed, seen = torch.from_numpy(c["holed"]), torch.from_numpy(c["seen"])
    before, missing_before = N.fill_missing(grid, holed, seen, k=c["k"])
    filled, missing = N.fill_missing(grid, holed, seen, k=c["k"], reach=c["reach"])
    assert missing_before.sum() >= 50 and not missing.any()
    assert torch.equal(filled[seen].view(torch.int16), holed[seen].view(torch.int16))
    was = ~missing_before
    assert torch.equal(filled[was].view(torch.int16), before[was].view(torch.int16))
    first, both = rr.fill_lists(c["xyz"], c["offsets"], 0.05, c["seen"], c["k"], c["reach"])
    ref, found = nr.blend(c["holed"], *both, "inverse", 0.05)
    unseen = ~c["seen"]
    assert found[unseen].all() and np.array_equal(filled.numpy()[unseen].view(np.uint16), ref[unseen].view(np.uint16))
    assert np.array_equal(missing_before.numpy(), unseen & (first[2] == 0))
    short, still = N.fill_missing(grid, holed, seen, k=c["k"], reach=1)      # reach 1: the middle of the strip stays open
    assert still.any() and still.sum() < missing_before.sum() and (short[still] == 0).all()


def test_refine_icp_with_reach_pairs_the_displaced_plane(monkeypatch):
    def moments(src, dst, xf12, tau2, dst_idx=None):
        inl, r2, m, _ = ar.moments(src.numpy(), dst.numpy(), np.asarray(xf12, dtype=np.float32), tau2, None if dst_idx is None else dst_idx.numpy())
        return torch.from_numpy(inl), torch.from_numpy(r2), torch.from_numpy(m)
    monkeypatch.setattr(ops, "rigid_moments", moments)
    c = rr.icp_case()
    index = N.PointIndex(grid_of(c["b"], [0, 800], 0.05))
    a = torch.from_numpy(c["a"])
    fit = align.refine_icp(index, a, align.RigidTransform(), iterations=10)
    assert not fit.ok and fit.count == 0 and (fit.neighbors == -1).all() and fit.iterations == 0
    first = align.refine_icp(index, a, align.RigidTransform(), iterations=0, reach=c["reach"])
    assert np.array_equal(first.neighbors.numpy(), rr.knn(c["b"], [0, 800], 0.05, c["a"], 0, 1, c["reach"])[0][:, 0]) and first.count == 800
    fit = align.refine_icp(index, a, align.RigidTransform(), iterations=10, reach=c["reach"])
    offset = float(np.abs(fit.transform.apply(c["a"])[:, 2].mean() - c["b"][:, 2].astype(np.float64).mean()))
    print("normal offset after ICP with reach: %.3g voxel sizes" % (offset / 0.05))
    assert fit.ok and fit.count == 800 and offset < 0.05


# ---------------------------------------------------------------------------------------------------- argument checks
def test_the_surface_refuses_bad_arguments():
    c = nr.two_scene_case()
    grid = grid_of(c["xyz"], c["offsets"], c["voxel_size"])
    index = N.PointIndex(grid)
    q = torch.from_numpy(c["queries"])
    mask = torch.zeros(300, dtype=torch.bool)
    for reach in (0, -1, 4097):
        with pytest.raises(ValueError):
            index.knn(q, 1, reach=reach)
        with pytest.raises(ValueError):
            index.knn_self(1, reach=reach)
        with pytest.raises(ValueError):
            R.distance_field(grid, mask, reach)
        with pytest.raises(ValueError):
            N.fill_missing(grid, torch.zeros((300, 2)), ~mask, reach=reach)
        with pytest.raises(ValueError):
            align.refine_icp(index, q, align.RigidTransform(), reach=reach)
    for reach in (2.0, "2", True):
        with pytest.raises(TypeError):
            index.knn(q, 1, reach=reach)
        with pytest.raises(TypeError):
            R.distance_field(grid, mask, reach)
    for radius in (0.0, -1.0, 0.3001, float("nan")):                         # (reach + 1) * voxel_size = 0.3
        with pytest.raises(ValueError):
            index.knn(q, 1, radius=radius, reach=2)
        with pytest.raises(ValueError):
            index.knn_self(1, radius=radius, reach=2)
        with pytest.raises(ValueError):
            N.fill_missing(grid, torch.zeros((300, 2)), ~mask, radius=radius, reach=2)
    index.knn(q, 1, radius=0.3, reach=2)
    with pytest.raises(ValueError):
        index.knn(q, 1, radius=0.1001)                                       # without reach the bound is what it was
    with pytest.raises(ValueError):
        R.distance_field(grid, torch.zeros(299, dtype=torch.bool), 2)       # a mask of the wrong length
    with pytest.raises(ValueError):
        R.distance_field(grid, mask, 2, per_voxel=True)                      # ... or over points where voxels are meant
    with pytest.raises(TypeError):
        R.distance_field(grid, mask.to(torch.uint8), 2)
    with pytest.raises(TypeError):
        R.distance_field("grid", mask, 2)
    with pytest.raises(ValueError):
        R.nearest_voxel(grid, q[:, :2], 0, mask, 2)
    with pytest.raises(TypeError):
        R.nearest_voxel(grid, q.long(), 0, mask, 2)
    with pytest.raises(TypeError):
        R.nearest_voxel(grid, q, torch.zeros(q.shape[0], dtype=torch.int32), mask, 2)
    with pytest.raises(ValueError):
        R.nearest_voxel(grid, q, torch.zeros(5, dtype=torch.int64), mask, 2)
    heat = torch.zeros((300, 2), dtype=torch.float16)
    with pytest.raises(TypeError):
        R.near(grid, heat.float(), 0, 1, 0.5, 0.2)
    with pytest.raises(ValueError):
        R.near(grid, heat[:299], 0, 1, 0.5, 0.2)
    with pytest.raises(IndexError):
        R.near(grid, heat, 2, 1, 0.5, 0.2)
    with pytest.raises(ValueError):
        R.near(grid, heat, 0, 1, 0.5, -0.1)
    with pytest.raises(ValueError):
        R.distance_field(grid, mask, 2).within(-1.0)


def test_the_wrapper_refuses_bad_arguments():
    q = torch.zeros((4, 4), dtype=torch.int32)
    src, ids = torch.zeros((3, 4), dtype=torch.int32), torch.arange(3, dtype=torch.int32)
    ok = dict(query_cells=q, source_cells=src, source_ids=ids, reach=4)
    for bad, exc in ((dict(query_cells=q.long()), TypeError), (dict(query_cells=q[:, :3]), ValueError), (dict(query_cells=q.reshape(-1)), ValueError),
                     (dict(source_cells=src.long()), TypeError), (dict(source_cells=src[:, :3]), ValueError), (dict(source_ids=ids.long()), TypeError),
                     (dict(source_ids=ids[:2]), ValueError), (dict(source_ids=ids[:, None]), ValueError), (dict(reach=0), ValueError),
                     (dict(reach=4097), ValueError), (dict(reach=1.5), TypeError), (dict(err=torch.zeros(2, dtype=torch.int32)), ValueError),
                     (dict(query_cells=[[0, 0, 0, 0]]), TypeError)):
        with pytest.raises(exc):
            REAL_REACH(**dict(ok, **bad))
    with pytest.raises(_lib.OpenSceneAmdError):                              # every check passed: only the device is missing
        REAL_REACH(**ok)
