"""openscene_amd.regions on the device against tests/regions_reference.py: the similarities inside the abs-sum bound of the
float64 dot products (nothing left out, -inf and NaN positions exact), the labelling EQUAL to the reference's components of
the device's own similarities, the records bit for bit, and the planted scenes end to end for both bank kinds."""
import numpy as np
import pytest
import torch

import regions_reference as rr

pytestmark = pytest.mark.gpu

VS = 0.05


def dev():
    return torch.device("cuda", 0)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---------------------------------------------------------------------------------------------------- edges
@pytest.mark.parametrize("connectivity", [26, 6])
@pytest.mark.parametrize("name", rr.edge_case_names())
def test_edges_inside_the_abs_sum_bound_of_the_float64_dot(name, connectivity):
    from openscene_amd import ops
    case = rr.edge_case(name)
    vox, nbr = case["vox"].to(dev()), torch.from_numpy(case["nbr"]).to(dev())
    sim = ops.regions_edges(vox, nbr, connectivity)
    again = ops.regions_edges(vox, nbr, connectivity)
    assert sim.dtype == torch.float32 and sim.shape == (ops.regions_n_off(connectivity), vox.shape[0])
    assert same_bits(sim, again)                                             # two calls, the same bits
    got = sim.cpu().numpy()
    want, bound = rr.edges_f64(case["vox"], case["nbr"], connectivity)
    ratio, bad, odd = rr.sim_errors(got, want, bound, rr.SIM_C)
    print("%s conn %d: worst error / abs-sum %.3e (SIM_C %.3e), %d beyond, %d -inf / NaN mismatches" % (name, connectivity, ratio, rr.SIM_C, bad, odd))
    assert odd == 0 and bad == 0
    assert bool(np.isneginf(got[:, case["isolated"]]).all())
    if case["nan_row"] is not None:
        ks = rr.offsets_of(connectivity)
        n, z = case["nan_row"], case["zero_row"]
        rows = np.arange(vox.shape[0])[None, :]
        present = case["nbr"][ks] >= 0
        assert np.array_equal(np.isnan(got), ((case["nbr"][ks] == n) | (rows == n)) & present)       # both sides, nothing else
        zero = ((case["nbr"][ks] == z) | (rows == z)) & present & ~np.isnan(got)
        assert bool((got[zero] == 0).all())


# ---------------------------------------------------------------------------------------------------- labelling
def centres(cells, vs=VS):
    return (torch.as_tensor(np.asarray(cells), dtype=torch.float64) + 0.5) * vs


def protos(d=16):
    return torch.linalg.qr(torch.randn(d, 4, generator=torch.Generator().manual_seed(2)))[0].t().contiguous()


def label_case(cells, proto_of_cell, offsets=None, connectivity=26, noise=0.05, seed=0):
    """One point per cell; the row of a voxel is its cell's prototype plus noise.  -> (grid, sim on the device, nbr numpy)"""
    from openscene_amd import ops
    from openscene_amd.objects import VoxelGrid
    grid = VoxelGrid(centres(cells).to(dev()), offsets, voxel_size=VS, connectivity=connectivity)
    assert grid.n_voxels == len(cells)
    cell_of_row = grid.coords.cpu()[:, 1:].tolist()
    gen = torch.Generator().manual_seed(seed)
    p = protos()
    rows = torch.stack([p[proto_of_cell(tuple(c))] for c in cell_of_row]) + noise * torch.randn(len(cells), p.shape[1], generator=gen)
    vox = torch.nn.functional.normalize(rows, dim=1).half().to(dev())
    return grid, ops.regions_edges(vox, grid.nbr, connectivity), grid.nbr.cpu().numpy()


def check_label(grid, sim, nbr, threshold, connectivity):
    """ops.regions_label == components() of the device's own sim: exact -> (voxel_root numpy, R)"""
    from openscene_amd import ops
    root = ops.regions_label(sim, grid.nbr, connectivity, threshold).cpu().numpy()
    want_root, _, r = rr.components(sim.cpu().numpy(), nbr, threshold, connectivity)
    assert root.dtype == np.int32 and np.array_equal(root, want_root)
    return root, r


def serpentine(length, rows):
    cells = []
    for r in range(rows):
        xs = range(length) if r % 2 == 0 else range(length - 1, -1, -1)
        cells += [(x, 2 * r, 0) for x in xs]
        if r + 1 < rows:
            cells.append((length - 1 if r % 2 == 0 else 0, 2 * r + 1, 0))
    return cells


@pytest.mark.parametrize("connectivity", [26, 6])
def test_a_snake_of_two_thousand_voxels_with_a_few_foreign_cells(connectivity):
    snake = serpentine(66, 30)                                               # 2009 voxels, one wide
    assert len(set(snake)) == len(snake) == 2009
    foreign = {snake[i] for i in (300, 301, 977, 1500)}
    perm = torch.randperm(len(snake), generator=torch.Generator().manual_seed(9)).tolist()
    cells = [snake[i] for i in perm]
    grid, sim, nbr = label_case(cells, lambda c: 1 if c in foreign else 0, connectivity=connectivity)
    root, r = check_label(grid, sim, nbr, 0.7, connectivity)
    assert (r == 7) if connectivity == 6 else (2 <= r <= 7)                  # four stretches and three foreign pieces; 26 may bridge a turn
    whole, r1 = check_label(grid, sim, nbr, -1.0, connectivity)             # every present edge: one region, root 0
    assert r1 == 1 and bool((whole == 0).all())


def test_a_dense_block_is_one_region_with_root_zero():
    cells = [(x, y, z) for x in range(12) for y in range(12) for z in range(12)]
    grid, sim, nbr = label_case(cells, lambda c: 2)
    root, r = check_label(grid, sim, nbr, 0.7, 26)
    assert r == 1 and bool((root == 0).all())


def test_a_checkerboard_is_two_regions_or_one_per_voxel():
    cells = [(x, y, z) for x in range(6) for y in range(6) for z in range(6)]
    for conn in (26, 6):
        grid, sim, nbr = label_case(cells, lambda c: (c[0] + c[1] + c[2]) % 2, connectivity=conn)
        root, r = check_label(grid, sim, nbr, 0.7, conn)
        assert r == (2 if conn == 26 else len(cells))
        if conn == 6:
            assert np.array_equal(root, np.arange(len(cells)))


def test_two_scenes_with_the_same_coordinates_and_features_never_merge():
    cells = [(x, y, z) for x in range(5) for y in range(5) for z in range(2)]
    grid, sim, nbr = label_case(cells + cells, lambda c: 0 if c[0] < 3 else 3, offsets=[0, len(cells), 2 * len(cells)], noise=0.0)
    root, r = check_label(grid, sim, nbr, 0.7, 26)
    assert r == 4
    scene = grid.coords.cpu()[:, 0].numpy()
    assert np.array_equal(scene[root], scene)


def test_a_threshold_equal_to_a_sim_unites_and_one_above_all_gives_every_voxel():
    case = rr.edge_case("24-plain")
    from openscene_amd import ops
    vox, nbr = case["vox"].to(dev()), torch.from_numpy(case["nbr"]).to(dev())
    sim = ops.regions_edges(vox, nbr, 26)
    s = sim.cpu().numpy()
    fin = np.isfinite(s)
    thr = float(np.sort(s[fin])[int(fin.sum() * 0.8)])                      # one of the sims, exactly (float32 -> float is exact)
    i, v = [int(a[0]) for a in np.nonzero(s == np.float32(thr))]
    root = ops.regions_label(sim, nbr, 26, thr).cpu().numpy()
    want_root, _, r = rr.components(s, case["nbr"], thr, 26)
    assert np.array_equal(root, want_root) and 1 < r < s.shape[1]
    assert root[v] == root[case["nbr"][i, v]]                                # >= unites the edge that sits on the threshold
    above = np.nextafter(np.float32(s[fin].max()), np.float32(np.inf))
    top = ops.regions_label(sim, nbr, 26, float(above)).cpu().numpy()
    assert np.array_equal(top, np.arange(s.shape[1]))


# ---------------------------------------------------------------------------------------------------- records
@pytest.mark.parametrize("n_regions", [0, 1, 37])
def test_records_of_an_arbitrary_labelling_bit_for_bit(n_regions):
    from openscene_amd import ops
    gen = torch.Generator().manual_seed(40 + n_regions)
    v_n, n = 301, 4099                                                       # more than one workgroup, no multiple of 64
    coords4 = torch.cat([torch.randint(0, 3, (v_n, 1), generator=gen), torch.randint(-300, 300, (v_n, 3), generator=gen)], 1).int()
    inverse = torch.randint(0, v_n, (n,), generator=gen).int()
    inverse[:700] = 5                                                        # a run of points on one record: the combined atomics
    xyz = (torch.randn(n, 3, generator=gen) * 10).float()
    xyz[3] = torch.tensor([-0.0, 0.0, -1e-30])
    region = torch.randint(-1, max(n_regions, 1), (v_n,), generator=gen).int().clamp(max=n_regions - 1)
    if n_regions:
        region[5] = n_regions - 1
    args = [t.to(dev()) for t in (xyz, inverse, coords4)]
    got = ops.regions_records(region.to(dev()), n_regions, *args)
    rr.assert_records(got, rr.records(region.numpy(), n_regions, xyz.numpy(), inverse.numpy(), coords4.numpy()))
    again = ops.regions_records(region.to(dev()), n_regions, *args)
    assert all(torch.equal(got[f], again[f]) for f in rr.RECORD_FIELDS)


def test_records_of_hand_made_waves_bit_for_bit():
    """objects_reference.wave_groups as regions: groups under, at and over the merge threshold, interleaved in their wave; a
    whole wave on one region; 64 regions in one wave; a short last wave with a lane whose voxel has region -1."""
    from objects_reference import wave_groups
    from openscene_amd import ops
    group = torch.from_numpy(wave_groups())
    n_regions = int(group.max()) + 1
    gen = torch.Generator().manual_seed(51)
    # two voxels per region and one voxel of region -1 (the last row), negative cells
    region = torch.cat([torch.arange(n_regions).repeat_interleave(2), torch.tensor([-1])]).int()
    v_n = region.shape[0]
    coords4 = torch.cat([torch.randint(0, 3, (v_n, 1), generator=gen), torch.randint(-300, -1, (v_n, 3), generator=gen)], 1).int()
    inverse = torch.where(group >= 0, 2 * group + torch.arange(group.shape[0]) % 2, torch.tensor(v_n - 1)).int()
    xyz = (torch.randn(group.shape[0], 3, generator=gen) * 10).float()
    xyz[70] = torch.tensor([-0.0, 0.0, -1e-30])                              # in the merged wave: both signs of the box words
    xyz[130] = torch.tensor([0.0, -0.0, -7.5])                               # on a lane that issues its own atomics
    assert group.shape[0] == 197 and int((region[inverse.long()] == -1).sum()) == 1
    got = ops.regions_records(region.to(dev()), n_regions, xyz.to(dev()), inverse.to(dev()), coords4.to(dev()))
    rr.assert_records(got, rr.records(region.numpy(), n_regions, xyz.numpy(), inverse.numpy(), coords4.numpy()))
    assert got["n_points"].cpu().tolist() == torch.bincount(group[group >= 0]).tolist()


@pytest.mark.parametrize("min_points", [1, 3])
def test_segment_numbers_filters_and_records_like_the_reference(min_points):
    from openscene_amd.objects import VoxelGrid
    from openscene_amd.regions import SimilarityGraph
    from openscene_amd.search import FeatureBank
    gen = torch.Generator().manual_seed(77)
    n = 3001
    xyz = (torch.rand(n, 3, generator=gen) * torch.tensor([3.0, 3.0, 0.6])).double()       # 5400 cells for 3001 points: many voxels hold one or two
    feats = torch.nn.functional.normalize(torch.randn(n, 16, generator=gen), dim=1).half()
    offsets = [0, 1700, n]
    bank = FeatureBank(16, dev())
    bank.add_scene("a", feats[:1700].to(dev()))
    bank.add_scene("b", feats[1700:].to(dev()))
    grid = VoxelGrid(xyz.to(dev()), offsets, voxel_size=0.1)
    graph = SimilarityGraph(bank, grid)
    s = graph.sim.cpu().numpy()
    thr = float(np.quantile(s[np.isfinite(s)], 0.7))                          # random rows: a mix of single voxels and larger pieces
    res = graph.segment(thr, min_points=min_points)
    ppv = torch.bincount(grid.inverse.cpu().long(), minlength=grid.n_voxels).numpy()
    _, region, r = rr.components(s, grid.nbr.cpu().numpy(), thr, 26, ppv, min_points)
    assert res.n_regions == r and np.array_equal(res.voxel_region.cpu().numpy(), region)
    pr = res.point_region.cpu()
    assert pr.dtype == torch.int32 and torch.equal(pr, torch.from_numpy(region)[grid.inverse.cpu().long()])
    assert res.n_dropped_points == int((pr == -1).sum()) and (res.n_dropped_points > 0) == (min_points == 3)
    rr.assert_records(res, rr.records(region, r, grid.xyz.cpu().numpy(), grid.inverse.cpu().numpy(), grid.coords.cpu().numpy()))
    cen = (res.vox_sum.double() / res.n_points.double()[:, None] + 0.5) * 0.1
    assert torch.equal(res.centroid, cen) and int(res.n_points.min()) >= min_points


# ---------------------------------------------------------------------------------------------------- end to end
def planted_on_device(dtype, perm=None):
    from openscene_amd.objects import VoxelGrid
    from openscene_amd.search import FeatureBank
    p = rr.planted()
    bank = FeatureBank(rr.PLANT_DIM, dev(), dtype=dtype)
    xyz = []
    for i, f in enumerate(p["feats"]):
        order = torch.arange(f.shape[0]) if perm is None else perm[i]
        bank.add_scene("scene%d" % i, f[order].to(dev()))
        xyz.append(p["xyz"][i][order].to(dev()))
    return p, bank, VoxelGrid.from_scenes(xyz, voxel_size=rr.PLANT_VOXEL)


@pytest.mark.parametrize("dtype", ["fp16", "fp8"])
def test_planted_scenes_end_to_end(dtype):
    from openscene_amd.regions import SimilarityGraph, segment
    p, bank, grid = planted_on_device(dtype)
    graph = SimilarityGraph(bank, grid, slice_voxels=500)
    sim, bits = graph.sim, graph.sim.clone()
    res = graph.segment(rr.PLANT_SIMILARITY, names=bank.names)
    planted_cls = rr.planted_check(graph, res, p["cls"])                     # margin, the float64 partition, pure regions
    classes, score = res.label(bank, p["protos"].half().to(dev()))
    assert torch.equal(classes.cpu(), planted_cls) and score.dtype == torch.float16 and float(score.float().min()) > 0.9
    assert torch.equal(res.point_labels(classes).cpu(), torch.cat(p["cls"]))
    # a second threshold reuses sim: the same tensor object, the same bits
    loose = graph.segment(-1.0)
    assert graph.sim is sim and same_bits(graph.sim, bits) and loose.n_regions == 3
    assert sorted(loose.scene.cpu().tolist()) == [0, 1, 2]
    assert sorted(r["id"] for r in res.regions("scene2")) == torch.nonzero(res.scene.cpu() == 2).reshape(-1).tolist() and len(res.regions(2)) == 6
    # the points of every scene permuted: the same partition as sets of points
    gen = torch.Generator().manual_seed(4)
    perm = [torch.randperm(f.shape[0], generator=gen) for f in p["feats"]]
    _, bank2, grid2 = planted_on_device(dtype, perm)
    res2 = segment(bank2, grid2, rr.PLANT_SIMILARITY)
    back = torch.empty_like(res2.point_region.cpu())
    whole = torch.cat([perm[i] + grid.offsets[i] for i in range(3)])
    back[whole] = res2.point_region.cpu()                                    # point whole[j] of the first order is point j of the second
    assert res2.n_regions == res.n_regions and rr.canonical(back) == rr.canonical(res.point_region.cpu())
    # a region as the next query finds its own points
    from openscene_amd.search import search
    q = res.descriptors(bank).queries()[7:8]
    hits = search(bank, q, thresholds=0.8, return_heat=True).heat[:, 0].float().cpu() >= 0.8
    assert torch.equal(hits, torch.cat(p["cls"]) == int(planted_cls[7]))


# ---------------------------------------------------------------------------------------------------- guards
def test_guards_raise_and_leave_the_bank_usable():
    from openscene_amd import _lib, ops
    from openscene_amd.objects import VoxelGrid
    from openscene_amd.regions import SimilarityGraph
    from openscene_amd.search import FeatureBank
    p, bank, grid = planted_on_device("fp16")
    good = SimilarityGraph(bank, grid)
    nbr = grid.nbr
    v = grid.n_voxels
    with pytest.raises(ValueError, match="multiple of 8"):
        ops.regions_edges(torch.zeros((v, 12), dtype=torch.float16, device=dev()), nbr)
    with pytest.raises(ValueError, match="1024"):
        ops.regions_edges(torch.zeros((v, 1032), dtype=torch.float16, device=dev()), nbr)
    with pytest.raises(TypeError):
        ops.regions_edges(torch.zeros((v, 16), dtype=torch.float32, device=dev()), nbr)
    for conn in (18, 0, 27):
        with pytest.raises(ValueError, match="connectivity"):
            ops.regions_edges(good.vox, nbr, conn)
        with pytest.raises(ValueError, match="connectivity"):
            ops.regions_label(good.sim, nbr, conn, 0.5)
    for bad in (float("nan"), float("inf"), float("-inf")):
        with pytest.raises(ValueError, match="finite"):
            good.segment(bad)
        with pytest.raises(ValueError, match="finite"):
            ops.regions_label(good.sim, nbr, 26, bad)
    short = FeatureBank(rr.PLANT_DIM, dev())
    short.add_scene("a", p["feats"][0].to(dev()))
    with pytest.raises(ValueError, match="rows"):
        SimilarityGraph(short, grid)
    host = VoxelGrid.__new__(VoxelGrid)                                      # a grid that claims another device
    host.__dict__.update(grid.__dict__)
    host.device = torch.device("cpu")
    with pytest.raises(ValueError, match="device"):
        SimilarityGraph(bank, host)
    with pytest.raises(ValueError):
        ops.regions_edges(good.vox, nbr.cpu())
    # a neighbour entry >= V: skipped (-inf), never dereferenced, and the err word turns into an exception
    broken = nbr.clone()
    broken[3, 10] = v
    broken[12, v - 1] = 2 ** 31 - 1
    with pytest.raises(_lib.OpenSceneAmdError, match="neighbour"):
        ops.regions_edges(good.vox, broken)
    err = torch.zeros(1, dtype=torch.int32, device=dev())
    sim = ops.regions_edges(good.vox, broken, 26, err=err)
    assert int(err.item()) == ops.REGIONS_E_NBR
    s, g = sim.cpu(), good.sim.cpu()
    assert s[3, 10] == float("-inf") and s[12, v - 1] == float("-inf")
    s[3, 10], s[12, v - 1] = g[3, 10], g[12, v - 1]
    assert same_bits(s, g)
    with pytest.raises(_lib.OpenSceneAmdError, match="neighbour"):
        ops.regions_label(good.sim, broken, 26, 0.7)
    with pytest.raises(_lib.OpenSceneAmdError, match="region"):
        ops.regions_records(torch.full((v,), 5, dtype=torch.int32, device=dev()), 3, grid.xyz, grid.inverse, grid.coords)
    with pytest.raises(_lib.OpenSceneAmdError, match="voxel row"):
        ops.regions_records(torch.zeros(v, dtype=torch.int32, device=dev()), 1, grid.xyz, torch.full_like(grid.inverse, v), grid.coords)
    # everything still works
    again = SimilarityGraph(bank, grid)
    assert same_bits(again.sim, good.sim) and again.segment(rr.PLANT_SIMILARITY).n_regions == 18
