"""openscene_amd.objects on the device against the numpy restatement of tests/objects_reference.py.  Every comparison is
exact: the fields are integers, selected input values, or derived from exact integers by the same host formula."""
import numpy as np
import pytest
import torch

import objects_reference as oref

pytestmark = pytest.mark.gpu

VS = 0.05


def dev():
    return torch.device("cuda", 0)


def centres(cells, vs=VS):
    return (torch.as_tensor(np.asarray(cells), dtype=torch.float64) + 0.5) * vs


def run(xyz, offsets, heat, thresholds, vs=VS, connectivity=26, min_points=1, max_objects=16):
    """find_objects on the device, checked field by field against the reference -> (result, reference dict)."""
    from openscene_amd.objects import VoxelGrid, find_objects
    grid = VoxelGrid(xyz.to(dev()), offsets, voxel_size=vs, connectivity=connectivity)
    res = find_objects(grid, heat.to(dev()), thresholds, min_points=min_points, max_objects=max_objects, return_point_ids=True)
    q = heat.shape[1]
    thr = np.broadcast_to(np.asarray(thresholds, dtype=np.float32).reshape(-1), (q,))
    ref = oref.find_objects(xyz, grid.offsets, heat, thr, voxel_size=vs, connectivity=connectivity, min_points=min_points,
                            max_objects=max_objects)
    oref.assert_same(res, ref, vs)
    # the member counts recomputed from the point ids equal n_points
    ids = res.point_object.cpu()
    for s in range(len(grid.offsets) - 1):
        a, b = grid.offsets[s], grid.offsets[s + 1]
        for j in range(q):
            col = ids[a:b, j]
            cnt = torch.bincount(col[col >= 0].long(), minlength=max_objects)
            assert torch.equal(cnt, res.n_points[s, j].cpu())
    return res, ref


def blobs(gen, n_blobs, pts_per_blob, spacing=8, sphere=False):
    """Blobs on a lattice `spacing` voxels apart.  A blob lies within the 3 x 3 x 3 voxels around its centre voxel, which holds
    the blob's first point: every voxel of a blob neighbours the centre (one object at connectivity 26), and two blobs never
    neighbour each other.  -> (positions in voxel units float64 [n, 3], blob id per point)"""
    side = int(np.ceil(n_blobs ** (1 / 3)))
    pos, bid = [], []
    for b in range(n_blobs):
        c = np.array([b % side, (b // side) % side, b // (side * side)], dtype=np.float64) * spacing - spacing
        u = torch.rand(pts_per_blob, 3, generator=gen, dtype=torch.float64).numpy() * 2 - 1          # [-1, 1)^3 voxels
        u[0] = 0.25                                                                                 # the centre voxel
        if sphere:
            u = u[np.linalg.norm(u, axis=1) < 1]
        pos.append(c + 0.5 + u)
        bid += [b] * u.shape[0]
    return np.concatenate(pos, 0), np.asarray(bid)


@pytest.mark.parametrize("q", [1, 20, 33])
def test_planted_boxes_and_spheres_have_the_known_count(q):
    gen = torch.Generator().manual_seed(q)
    n_blobs = 11
    pos, bid = blobs(gen, n_blobs, 97, sphere=(q == 20))
    noise = torch.rand(1000 + q, 3, generator=gen, dtype=torch.float64).numpy() * 40 - 12
    xyz = torch.from_numpy(np.concatenate([pos, noise], 0)) * VS
    n = xyz.shape[0]
    if n % 64 == 0:
        xyz = xyz[:-1]
        n -= 1
    perm = torch.randperm(n, generator=gen)
    xyz, bid_all = xyz[perm], torch.from_numpy(np.concatenate([bid, np.full(noise.shape[0], -1)]))[perm][:n]
    wanted = torch.rand(q, n_blobs, generator=gen) < 0.5                    # the blobs each query lights up
    heat = torch.rand(n, q, generator=gen) * 0.4                            # everything else stays below 0.5
    for j in range(q):
        lit = (bid_all >= 0) & wanted[j][bid_all.clamp(min=0)]
        heat[lit, j] = 0.5 + torch.rand(int(lit.sum()), generator=gen) * 0.5
    res, _ = run(xyz, None, heat.half(), 0.5, max_objects=16)
    assert res.n_objects[0].cpu().tolist() == wanted.sum(1).tolist()


@pytest.mark.parametrize("shift,n26,n6", [((0, 0, 0), 1, 2), ((0, 0, -2), 1, 2), ((0, -2, -2), 1, 1), ((1, 0, 0), 2, 2)])
def test_blobs_touching_across_an_edge_or_a_corner(shift, n26, n6):
    """Two 2 x 2 x 2 cubes: [-2, -1]^3 and [0, 1]^3 moved by `shift` -- corner to corner, along an edge, face to face, apart."""
    a = [(x, y, z) for x in (-2, -1) for y in (-2, -1) for z in (-2, -1)]
    b = [(x + shift[0], y + shift[1], z + shift[2]) for x in (0, 1) for y in (0, 1) for z in (0, 1)]
    xyz = centres(a + b)
    heat = torch.full((len(a) + len(b), 2), 1.0, dtype=torch.float16)
    for conn, want in ((26, n26), (6, n6)):
        res, _ = run(xyz, None, heat, 0.5, connectivity=conn)
        assert res.n_objects.cpu().tolist() == [[want, want]]


def serpentine(length, rows):
    cells = []
    for r in range(rows):
        xs = range(length) if r % 2 == 0 else range(length - 1, -1, -1)
        cells += [(x, 2 * r, 0) for x in xs]
        if r + 1 < rows:
            cells.append((length - 1 if r % 2 == 0 else 0, 2 * r + 1, 0))
    return cells


@pytest.mark.parametrize("shuffle", [False, True])
def test_serpentine_corridor_is_one_object_and_the_gap_stays_open(shuffle):
    snake = serpentine(100, 60)
    assert len(snake) == 6059 and len(set(snake)) == 6059
    fence = [(101, y, 0) for y in range(-3, 125)]                           # two voxels from the turns: not a neighbour
    cells = np.asarray(snake + fence)
    gen = torch.Generator().manual_seed(5)
    if shuffle:
        cells = cells[torch.randperm(len(cells), generator=gen).numpy()]
    xyz = centres(cells)
    heat = (0.5 + 0.25 * torch.rand(len(cells), 3, generator=gen)).half()
    heat[:, 2] = 0.0
    for conn in (26, 6):
        res, _ = run(xyz, None, heat, [0.5, 0.25, 0.5], connectivity=conn, max_objects=4)
        assert res.n_objects.cpu().tolist() == [[2, 2, 0]]
        assert sorted(res.n_voxels[0, 0, :2].cpu().tolist()) == [128, 6059]
        assert res.n_voxels[0, 0, 2:].eq(0).all()
    # odd rows filled in: the corridor's folds now touch and the fence is still apart
    filled = np.asarray(list(set(snake) | {(x, y, 0) for x in range(100) for y in range(1, 119, 2)}) + fence)
    res, _ = run(centres(filled), None, torch.ones(len(filled), 1, dtype=torch.float16), 0.5)
    assert res.n_objects.item() == 2


def test_scenes_never_merge_and_empty_scenes_pad():
    gen = torch.Generator().manual_seed(7)
    pos, _ = blobs(gen, 3, 50)
    one = torch.from_numpy(pos) * VS
    heat_one = (torch.rand(one.shape[0], 4, generator=gen)).half()
    xyz = torch.cat([one, one, one, torch.rand(37, 3, dtype=torch.float64, generator=gen)], 0)
    n1 = one.shape[0]
    offsets = [0, n1, n1, 2 * n1, 3 * n1, 3 * n1 + 37]                       # scene 1 has no points, scene 3 and 4 no hits
    heat = torch.cat([heat_one, heat_one, torch.zeros(n1, 4, dtype=torch.float16), torch.full((37, 4), -1.0, dtype=torch.float16)], 0)
    res, _ = run(xyz, offsets, heat, 0.25, max_objects=8)
    for f in oref.FIELDS:
        assert torch.equal(getattr(res, f)[0], getattr(res, f)[2]), f          # identical scenes: identical, separate objects
    assert (res.n_objects[0] > 0).all()
    for s in (1, 3, 4):
        assert res.n_objects[s].eq(0).all() and res.n_points[s].eq(0).all() and res.peak_point[s].eq(-1).all()
        assert torch.isinf(res.peak_score[s].float()).all() and (res.peak_score[s] < 0).all()
    assert res.point_object[2 * n1:].eq(-1).all()


def test_score_edge_cases_nan_inf_threshold_and_per_query_thresholds():
    cells = [(i, 0, 0) for i in range(12)]
    xyz = centres(cells)
    inf, nan = float("inf"), float("nan")
    col = [0.5, nan, 0.75, inf, 0.5, -inf, 0.5, 0.4998, 0.5, 0.25, -0.0, 0.0]
    heat = torch.tensor([col, col, [nan] * 12], dtype=torch.float16).t().contiguous()
    res, _ = run(xyz, None, heat, [0.5, 0.0, 0.0])
    # query 0: {0}, {2}, {4}, {6}, {8}: NaN / +inf / -inf split the row and are never members; 0.5 == the threshold is a member
    assert res.n_objects.cpu().tolist() == [[5, 4, 0]]
    assert res.n_points[0, 0, :5].cpu().tolist() == [1] * 5 and res.peak_point[0, 0, :5].cpu().tolist() == [2, 0, 4, 6, 8]
    # query 1 at 0.0: {0}, {2}, {4}, {6 .. 11} with -0.0 >= 0.0 a member
    assert sorted(res.n_points[0, 1, :4].cpu().tolist()) == [1, 1, 1, 6]
    assert res.point_object[:, 2].eq(-1).all() and res.point_object[[1, 3, 5], :].eq(-1).all()
    res, _ = run(xyz, None, heat, [inf, nan, -inf])
    assert res.n_objects.cpu().tolist() == [[0, 0, 0]]


def test_negative_coordinates_and_points_on_voxel_faces():
    gen = torch.Generator().manual_seed(11)
    vs = 0.25                                                                # faces are exact in binary
    k = torch.randint(-40, 40, (3001, 3), generator=gen).double()
    xyz = k * vs                                                             # every point ON a voxel face (and edge, and corner)
    xyz[::3] += torch.rand(1001, 3, generator=gen, dtype=torch.float64) * vs
    xyz[1::7] = -xyz[1::7]
    heat = torch.rand(3001, 5, generator=gen).half()
    run(xyz, None, heat, [0.9, 0.8, 0.7, 0.6, 0.5], vs=vs, max_objects=32)
    run(xyz.float(), [0, 1000, 3001], heat, 0.7, vs=vs, connectivity=6, max_objects=32)


def test_cap_min_points_and_equal_peaks():
    gen = torch.Generator().manual_seed(13)
    pos, bid = blobs(gen, 40, 9, spacing=6)
    xyz = torch.from_numpy(pos) * VS
    n = xyz.shape[0]
    heat = torch.zeros(n, 3)
    heat[:, 0] = 0.5 + torch.rand(n, generator=gen) * 0.5
    heat[:, 1] = 0.75                                                        # every peak equal: ordered by the peak's row
    heat[:, 2] = heat[:, 0]
    heat[torch.from_numpy(bid) % 2 == 1, 2] = 0.0                            # half the blobs: one point each over the threshold
    heat[torch.from_numpy(np.r_[True, bid[1:] != bid[:-1]]), 2] = 0.625
    res, ref = run(xyz, None, heat.half(), 0.5, max_objects=8)
    assert res.n_objects.cpu().tolist() == [[40, 40, 40]]
    assert (ref["point_object"][:, 0] == -1).sum() == (ref["n_points"][0, 0].sum() - n).abs()        # past the cap: -1
    first_rows = [int(np.nonzero(bid == b)[0][0]) for b in range(8)]
    assert res.peak_point[0, 1].cpu().tolist() == first_rows and res.peak_score[0, 1].eq(0.75).all()
    res, _ = run(xyz, None, heat.half(), 0.5, min_points=2, max_objects=64)
    assert res.n_objects.cpu().tolist() == [[40, 40, 20]]
    res, _ = run(xyz, None, heat.half(), 0.5, min_points=10, max_objects=1)
    assert res.n_objects.cpu().tolist() == [[0, 0, 0]] and res.point_object.eq(-1).all()


def test_fifty_thousand_hits_on_one_record_and_duplicate_points():
    gen = torch.Generator().manual_seed(17)
    # a 5 x 5 floor of voxels with 2 000 points each, duplicates included, in scan order: every wave targets one record
    cells = torch.randint(0, 5, (50_000, 2), generator=gen)
    xyz = torch.cat([(cells.double() + torch.rand(50_000, 2, generator=gen, dtype=torch.float64)) * VS,
                     torch.full((50_000, 1), 0.01, dtype=torch.float64)], 1)
    xyz[1000:2000] = xyz[:1000]                                              # exact duplicates
    extra = centres([(20, 20, 20)] * 64 + [(30, 30, 30)])                    # 64 points in one voxel, and a lone one
    xyz = torch.cat([xyz, extra], 0)
    heat = torch.rand(xyz.shape[0], 2, generator=gen).half()
    heat[:, 1] = (heat[:, 1].float() * 60000).half()                         # raw scores near the fp16 maximum, negatives too
    heat[::5, 1] = -heat[::5, 1]
    res, _ = run(xyz, None, heat, [0.0, -70000.0], max_objects=4)
    assert res.n_objects.cpu().tolist() == [[3, 3]]
    for j in range(2):
        assert sorted(res.n_points[0, j, :3].cpu().tolist()) == [1, 64, 50_000]
        assert sorted(res.n_voxels[0, j, :3].cpu().tolist()) == [1, 1, 25]


def test_hand_made_waves_with_and_without_the_wave_combine():
    """objects_reference.wave_groups as connected components: every group in one or two voxels of its own, three voxels from the
    next group's, every score over the threshold except on the lane that is left out.  33 queries: a full tile of 32 and a
    tile of one.  Each wave is a scene of its own kind: 64 objects is the most a (scene, query) returns."""
    from openscene_amd import ops
    from openscene_amd.objects import VoxelGrid
    group = oref.wave_groups()
    n, q = group.shape[0], 33
    gen = torch.Generator().manual_seed(37)
    g = np.where(group >= 0, group, group.max() + 1)                         # the left-out lane: a voxel of its own
    cell = np.stack([3 * (g % 9) - 12 + np.arange(n) % 2, 3 * (g // 9) - 12, np.full(n, -5)], 1)
    xyz = (torch.from_numpy(cell).double() + 0.5 + (torch.rand(n, 3, generator=gen, dtype=torch.float64) - 0.5) * 0.6) * VS
    heat = (0.5 + 0.5 * torch.rand(n, q, generator=gen)).half()
    heat[group < 0] = 0.25
    offsets = [0, 128, 192, n]
    res, _ = run(xyz, offsets, heat, 0.5, max_objects=64)
    assert res.n_objects.cpu().tolist() == [[6] * q, [64] * q, [1] * q]
    grid = VoxelGrid(xyz.to(dev()), offsets, voxel_size=VS)
    thr = torch.full((q,), 0.5, device=dev())
    both = [ops.objects_find(heat.to(dev()), thr, grid.xyz, grid.inverse, grid.coords, grid.nbr, grid.offsets_tensor(), max_objects=64,
                             return_point_ids=True, combine=combine) for combine in (True, False)]
    for f in oref.FIELDS + ("n_objects", "point_object"):
        a, b = both[0][f], both[1][f]
        assert a.dtype == b.dtype and a.shape == b.shape, f
        assert torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), f
        assert torch.equal(a, getattr(res, f)), f


def test_repeatable_bit_for_bit_also_after_unrelated_work():
    from openscene_amd.objects import VoxelGrid, find_objects
    gen = torch.Generator().manual_seed(19)
    xyz = (torch.rand(40_001, 3, generator=gen, dtype=torch.float64) * 3).to(dev())
    heat = torch.rand(40_001, 9, generator=gen).half().to(dev())
    grid = VoxelGrid(xyz, [0, 15_000, 40_001], voxel_size=VS)
    first = find_objects(grid, heat, 0.6, max_objects=32, return_point_ids=True)
    again = find_objects(grid, heat, 0.6, max_objects=32, return_point_ids=True)
    junk = torch.randn(1024, 1024, device=dev())
    for _ in range(5):
        junk = junk @ junk * 1e-3
    third = find_objects(VoxelGrid(xyz, [0, 15_000, 40_001], voxel_size=VS), heat, 0.6, max_objects=32, return_point_ids=True)
    for other in (again, third):
        for f in oref.FIELDS + ("n_objects", "point_object", "mean_score", "centroid"):
            a, b = getattr(first, f), getattr(other, f)
            if a.dtype == torch.float16:
                a, b = a.view(torch.int16), b.view(torch.int16)
            elif a.dtype == torch.float32:
                a, b = a.view(torch.int32), b.view(torch.int32)
            elif a.dtype == torch.float64:
                a, b = a.view(torch.int64), b.view(torch.int64)
            assert torch.equal(a, b), f
    assert first.n_objects.sum().item() > 100


def test_voxel_row_order_is_not_observable():
    from openscene_amd.objects import VoxelGrid, find_objects
    gen = torch.Generator().manual_seed(23)
    n = 20_003
    xyz = torch.rand(n, 3, generator=gen, dtype=torch.float64) * 2
    heat = torch.rand(n, 4, generator=gen).half()
    thr = [0.55, 0.9, 0.997, 0.999]
    base = find_objects(VoxelGrid(xyz.to(dev()), voxel_size=VS), heat.to(dev()), thr, max_objects=64)
    perm = torch.randperm(n, generator=gen)                                  # another point order: another voxel row order
    moved = find_objects(VoxelGrid(xyz[perm].to(dev()), voxel_size=VS), heat[perm].to(dev()), thr, max_objects=64)
    assert torch.equal(base.n_objects, moved.n_objects)
    compared = 0
    for j in range(4):
        if base.n_objects[0, j].item() > 64:
            continue                                                          # (equal peaks are ordered by ROW: the cap may cut elsewhere)
        compared += 1
        pp = moved.peak_point[0, j].cpu()
        back = torch.where(pp >= 0, perm[pp.clamp(min=0)], pp)               # the peak's row in the first order
        a = sorted(zip(base.n_points[0, j].tolist(), base.n_voxels[0, j].tolist(), base.score_sum[0, j].tolist(),
                       base.vox_sum[0, j].tolist(), base.box_min[0, j].tolist(), base.peak_score[0, j].tolist()))
        b = sorted(zip(moved.n_points[0, j].tolist(), moved.n_voxels[0, j].tolist(), moved.score_sum[0, j].tolist(),
                       moved.vox_sum[0, j].tolist(), moved.box_min[0, j].tolist(), moved.peak_score[0, j].tolist()))
        assert a == b
        assert torch.equal(heat[back[pp >= 0], j], moved.peak_score[0, j].cpu()[pp >= 0])
    assert compared >= 1


def test_out_of_range_coordinate_raises_and_names_the_range():
    from openscene_amd.objects import VoxelGrid
    xyz = torch.tensor([[0.0, 0.0, 0.0], [0.0, 40000 * VS, 0.0]], dtype=torch.float64, device=dev())
    with pytest.raises(ValueError, match="32767"):
        VoxelGrid(xyz, voxel_size=VS)
    with pytest.raises(ValueError, match="32767"):
        VoxelGrid(-xyz, voxel_size=VS)


def test_eight_scenes_of_the_s100k_room_searched_by_planted_directions():
    from openscene_amd import synthetic as syn
    from openscene_amd.objects import VoxelGrid
    from openscene_amd.search import FeatureBank, search
    d, q_n, s_n = 64, 8, 8
    gen = torch.Generator().manual_seed(29)
    room = torch.from_numpy(syn.room_points(0))                              # the S100k scene's 120 000 points
    n1 = room.shape[0]
    directions = torch.nn.functional.normalize(torch.randn(q_n, d, generator=gen), dim=1)
    bank = FeatureBank(d, dev(), capacity_rows=s_n * n1)
    scenes = []
    for s in range(s_n):
        xyz = room + torch.tensor([5.0 * (s % 4), 4.0 * (s // 4), 0.0], dtype=torch.float64)       # tiled 4 x 2
        feats = torch.randn(n1, d, generator=gen) * 0.25
        for j in range(q_n):                                                 # query j: a few balls of its direction per scene
            for _ in range(1 + (s + j) % 3):
                c = room[int(torch.randint(0, n1, (1,), generator=gen))]
                near = (room - c).norm(dim=1) < 0.12 + 0.04 * j
                feats[near] += directions[j] * (2.0 + torch.rand(int(near.sum()), 1, generator=gen))
        bank.add_scene("room%d" % s, feats.to(dev()))
        scenes.append(xyz)
    xyz = torch.cat(scenes, 0)
    grid = VoxelGrid(xyz.to(dev()), bank.offsets, voxel_size=0.02)
    res = search(bank, directions.half().to(dev()), k=4, thresholds=0.6, return_heat=True)
    found = res.find_objects(grid, 0.6, min_points=3, max_objects=12, return_point_ids=True)
    ref = oref.find_objects(xyz, bank.offsets, res.heat, [0.6] * q_n, voxel_size=0.02, min_points=3, max_objects=12)
    oref.assert_same(found, ref, 0.02)
    assert found.names == bank.names and (found.n_objects > 0).float().mean().item() > 0.9
    assert found.rank_scenes(0)[0][1] == int(found.n_objects[:, 0].max())
