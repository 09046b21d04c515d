"""openscene_amd.merge on the device against tests/merge_reference.py: the contacts exact, the pair similarities bit for bit
those of ops.regions_edges on the same rows and inside the abs-sum bound of the float64 dot products, a round's parents EQUAL
to the reference's round, the fold bit for bit the sequential float32 adds, and the planted scenes, the strip and the corner
contact end to end."""
import os
import re

import numpy as np
import pytest
import torch

import merge_reference as mr
import regions_reference as rr

pytestmark = pytest.mark.gpu

CUT = 0.995


def dev():
    return torch.device("cuda", 0)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def i32(x):
    return torch.as_tensor(np.asarray(x), dtype=torch.int32).reshape(-1).to(dev())


# ---------------------------------------------------------------------------------------------------- contacts
def random_labelling(v_n, n_regions, seed):
    gen = torch.Generator().manual_seed(seed)
    region = torch.randint(-1, n_regions, (v_n,), generator=gen).int()
    region[:n_regions] = torch.arange(n_regions).int()                        # every region occurs
    return region


@pytest.mark.parametrize("connectivity", [26, 6])
@pytest.mark.parametrize("name", ["8-plain", "24-special"])
def test_contacts_of_a_random_labelling_are_exact(name, connectivity):
    from openscene_amd import ops
    case = rr.edge_case(name)
    v_n = case["nbr"].shape[1]
    assert v_n % 256 != 0 and v_n > 256                                       # more than one workgroup, the last one short
    region = random_labelling(v_n, 23, 60 + connectivity)
    assert int((region == -1).sum()) > 0
    nbr = torch.from_numpy(case["nbr"]).to(dev())
    key = ops.regions_contacts(region.to(dev()), nbr, connectivity, 23)
    want, bits = mr.contact_keys(region.numpy(), case["nbr"], connectivity, 23)
    assert bits == 0 and key.dtype == torch.int64 and np.array_equal(key.cpu().numpy(), want) and int((want >= 0).sum()) > 100
    one = ops.regions_contacts(torch.zeros(v_n, dtype=torch.int32, device=dev()), nbr, connectivity, 1)
    assert bool((one == -1).all())                                           # one region: no contacts


def test_region_adjacency_and_its_guards():
    from openscene_amd import _lib, ops
    from openscene_amd.merge import region_adjacency
    from openscene_amd.objects import VoxelGrid
    case = rr.edge_case("24-plain")
    cells = torch.from_numpy(case["coords4"][:, 1:].astype(np.float64))
    grid = VoxelGrid(((cells + 0.5) * 0.05).to(dev()), None, voxel_size=0.05)
    v_n = grid.n_voxels
    assert v_n == case["nbr"].shape[1]
    region = random_labelling(v_n, 40, 7)
    lo, hi, c = region_adjacency(grid, region.to(dev()), 40)
    wlo, whi, wc = mr.adjacency(region.numpy(), grid.nbr.cpu().numpy(), 26, 40)
    assert lo.dtype == torch.int32 and c.dtype == torch.int64
    assert np.array_equal(lo.cpu().numpy(), wlo) and np.array_equal(hi.cpu().numpy(), whi) and np.array_equal(c.cpu().numpy(), wc)
    assert bool((lo < hi).all()) and len(wlo) > 100
    # a region id >= n_regions: the bit, the entry skipped, the check raises
    bad = region.clone()
    bad[17] = 40
    err = torch.zeros(1, dtype=torch.int32, device=dev())
    key = ops.regions_contacts(bad.to(dev()), grid.nbr, 26, 40, err=err)
    assert int(err.item()) == ops.REGIONS_E_REGION
    want, bits = mr.contact_keys(bad.numpy(), grid.nbr.cpu().numpy(), 26, 40)
    assert bits == mr.E_REGION and np.array_equal(key.cpu().numpy(), want)
    k = key.cpu().numpy()
    assert bool(((k[k >= 0] >> 32) < 40).all()) and bool(((k[k >= 0] & 0xFFFFFFFF) < 40).all())
    with pytest.raises(_lib.OpenSceneAmdError, match="region"):
        ops.regions_contacts(bad.to(dev()), grid.nbr, 26, 40)
    with pytest.raises(_lib.OpenSceneAmdError, match="region"):
        region_adjacency(grid, bad.to(dev()), 40)


# ---------------------------------------------------------------------------------------------------- pair dot
@pytest.mark.parametrize("name", rr.edge_case_names())
def test_pair_dot_gives_the_bits_of_the_edge_kernel_inside_the_float64_bound(name):
    from openscene_amd import ops
    case = rr.edge_case(name)
    vox, nbr = case["vox"].to(dev()), torch.from_numpy(case["nbr"]).to(dev())
    edges = ops.regions_edges(vox, nbr, 26).cpu()
    i, v = np.nonzero(case["nbr"][:13] >= 0)
    u = case["nbr"][:13][i, v]
    lo, hi = np.minimum(v, u), np.maximum(v, u)
    order = np.lexsort((hi, lo))                                             # the list as merge_regions makes it: ascending (lo, hi)
    lo, hi, i, v = lo[order], hi[order], i[order], v[order]
    sim = ops.rows_pair_dot(vox, i32(lo), i32(hi))
    again = ops.rows_pair_dot(vox, i32(lo), i32(hi))
    assert sim.dtype == torch.float32 and sim.shape == (len(lo),) and same_bits(sim, again)
    assert same_bits(sim.cpu(), edges[torch.from_numpy(i), torch.from_numpy(v)])          # the same two rows, the same bits
    assert same_bits(ops.rows_pair_dot(vox, i32(hi), i32(lo)), sim)                        # ... whichever is lo
    got = sim.cpu().numpy()
    want, bound = mr.pair_sims_f64(case["vox"], lo, hi)
    ratio, bad, odd = rr.sim_errors(got, want, bound, rr.SIM_C)
    print("%s: %d pairs, worst error / abs-sum %.3e (SIM_C %.3e), %d beyond, %d -inf / NaN mismatches" % (name, len(lo), ratio, rr.SIM_C, bad, odd))
    assert odd == 0 and bad == 0 and len(lo) > 1000
    if case["nan_row"] is not None:
        n = case["nan_row"]
        assert np.array_equal(np.isnan(got), (lo == n) | (hi == n)) and np.isnan(got).sum() > 0


def test_pair_dot_shapes_around_the_run_length():
    from openscene_amd import _lib, ops
    run = ops.MERGE_RUN
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "openscene_amd", "csrc", "merge.hip")).read()
    assert int(re.search(r"constexpr int MERGE_RUN = (\d+);", src).group(1)) == run
    case = rr.edge_case("768-plain")
    vox = case["vox"].to(dev())
    r_n = vox.shape[0]
    # all pairs of 40 rows: row 0 has 39 partners, more than three runs; the table every other list is compared with
    a, b = np.triu_indices(40, 1)
    assert 39 > 3 * run
    dense = ops.rows_pair_dot(vox, i32(a), i32(b)).cpu()
    table = torch.zeros(40, 40)
    table[torch.from_numpy(a), torch.from_numpy(b)] = dense
    want, bound = mr.pair_sims_f64(case["vox"], a, b)
    ratio, bad, odd = rr.sim_errors(dense.numpy(), want, bound, rr.SIM_C)
    assert bad == 0 and odd == 0
    gen = torch.Generator().manual_seed(12)
    lists = {"one-lo": (np.zeros(39, dtype=np.int64), np.arange(1, 40)),
             "lo-changes-at-every-pair": (np.arange(39), np.arange(1, 40)),
             "a-repeated-pair": (np.array([3, 3, 3, 2, 3]), np.array([7, 7, 7, 9, 7]))}
    perm = torch.randperm(len(a), generator=gen).numpy()
    lists["unsorted"] = (a[perm], b[perm])
    for e in (0, 1, run - 1, run, run + 1, 2 * run + 3):
        lists["first-%d" % e] = (a[:e], b[:e])
    for what, (lo, hi) in lists.items():
        sim = ops.rows_pair_dot(vox, i32(lo), i32(hi)).cpu()
        assert sim.shape == (len(lo),) and same_bits(sim, table[torch.from_numpy(lo).long(), torch.from_numpy(hi).long()]), what
    # 1000 pairs over all rows, not a multiple of the run length times the waves of a workgroup
    lo = torch.randint(0, r_n, (1000,), generator=gen).numpy()
    hi = torch.randint(0, r_n, (1000,), generator=gen).numpy()
    sim = ops.rows_pair_dot(vox, i32(lo), i32(hi))
    want, bound = mr.pair_sims_f64(case["vox"], lo, hi)
    ratio, bad, odd = rr.sim_errors(sim.cpu().numpy(), want, bound, rr.SIM_C)
    assert bad == 0 and odd == 0 and same_bits(sim, ops.rows_pair_dot(vox, i32(lo), i32(hi)))
    # an end out of range: -inf, the bit, the others untouched; the check raises
    blo, bhi = lo.copy(), hi.copy()
    blo[5], bhi[77], blo[999] = -1, r_n, 2 ** 31 - 1
    err = torch.zeros(1, dtype=torch.int32, device=dev())
    broken = ops.rows_pair_dot(vox, i32(blo), i32(bhi), err=err).cpu()
    assert int(err.item()) == ops.REGIONS_E_PAIR
    assert broken[5] == broken[77] == broken[999] == float("-inf")
    good = sim.cpu().clone()
    good[[5, 77, 999]] = float("-inf")
    assert same_bits(broken, good)
    with pytest.raises(_lib.OpenSceneAmdError, match="pair end"):
        ops.rows_pair_dot(vox, i32(blo), i32(bhi))
    assert same_bits(ops.rows_pair_dot(vox, i32(lo), i32(hi)), sim)          # everything still works


# ---------------------------------------------------------------------------------------------------- round
def check_round(lo, hi, sim, n_regions, threshold):
    from openscene_amd import ops
    s = torch.as_tensor(np.asarray(sim, dtype=np.float32)).reshape(-1).to(dev())
    parent = ops.regions_merge_round(i32(lo), i32(hi), s, n_regions, threshold)
    want, bits = mr.merge_round(lo, hi, np.asarray(sim, dtype=np.float32), n_regions, threshold)
    assert bits == 0 and parent.dtype == torch.int32 and parent.cpu().tolist() == want
    return want


def test_rounds_on_hand_made_lists():
    nan, ninf = float("nan"), float("-inf")
    below = float(np.nextafter(np.float32(0.5), np.float32(0)))
    # ties on equal sims: the lower edge index wins from both ends
    assert check_round([0, 1], [1, 2], [0.9, 0.9], 3, 0.5) == [0, 0, 0]
    assert check_round([0, 1, 1], [2, 2, 3], [0.9, 0.9, 0.9], 4, 0.5) == [0, 0, 0, 3]       # 3 names (1, 3), 1 names (1, 2): not mutual
    # below the threshold, equal to it, NaN, -inf
    assert check_round([0, 2, 4, 6], [1, 3, 5, 7], [0.5, below, nan, ninf], 8, 0.5) == [0, 0, 2, 3, 4, 5, 6, 7]
    # -0 orders below +0: region 1 prefers its +0 edge although the index is higher; (0, 3) is a mutual pair of its own
    assert check_round([0, 0, 1], [1, 3, 2], [-0.0, 0.5, 0.0], 4, -1.0) == [0, 1, 1, 0]
    assert check_round([0, 0, 1], [1, 3, 2], [0.0, 0.5, -0.0], 4, -1.0) == [0, 0, 2, 0]
    # a chain a -> b -> c -> d with (c, d) mutual: b joins, a does not
    assert check_round([0, 1, 2], [1, 2, 3], [0.6, 0.7, 0.8], 4, 0.5) == [0, 1, 1, 1]
    # 70 regions pointing at one mutual pair: more than a wave
    lo = [0] + [0 if j % 2 else 1 for j in range(70)]
    hi = [1] + list(range(2, 72))
    want = check_round(lo, hi, [0.99] + [0.9 - 0.001 * j for j in range(70)], 75, 0.5)
    assert want == [0] * 72 + [72, 73, 74]                                   # (and three isolated regions)
    # two disjoint mutual pairs joined by a weaker edge that neither end names
    assert check_round([0, 1, 3], [1, 3, 4], [0.9, 0.6, 0.8], 6, 0.5) == [0, 0, 2, 3, 3, 5]
    # R = 1, E = 0
    assert check_round([], [], [], 1, 0.5) == [0]
    assert check_round([], [], [], 5, 0.5) == [0, 1, 2, 3, 4]
    # a few hundred random edges with many ties
    gen = torch.Generator().manual_seed(31)
    e = 900
    a, b = torch.randint(0, 300, (e,), generator=gen), torch.randint(0, 300, (e,), generator=gen)
    keep = a != b
    lo, hi = torch.minimum(a, b)[keep].tolist(), torch.maximum(a, b)[keep].tolist()
    sim = (torch.randint(0, 12, (len(lo),), generator=gen).float() / 10).tolist()
    want = check_round(lo, hi, sim, 300, 0.45)
    assert 1 < len(set(want)) < 300


def test_round_guards():
    from openscene_amd import _lib, ops
    sim = torch.tensor([0.9, 0.9, 0.9], device=dev())
    err = torch.zeros(1, dtype=torch.int32, device=dev())
    parent = ops.regions_merge_round(i32([0, 1, 2]), i32([1, 7, 3]), sim, 4, 0.5, err=err)
    assert int(err.item()) == ops.REGIONS_E_PAIR and parent.cpu().tolist() == [0, 0, 2, 2]           # the bad pair skipped
    with pytest.raises(_lib.OpenSceneAmdError, match="pair end"):
        ops.regions_merge_round(i32([0, 1, 2]), i32([1, -1, 3]), sim, 4, 0.5)
    lib = _lib.load()
    assert lib.osn_merge_ws_bytes(10) == 80 and lib.osn_merge_ws_bytes(0) == 0


# ---------------------------------------------------------------------------------------------------- fold
@pytest.mark.parametrize("d", [8, 520, 768, 1024])
def test_fold_is_the_sequential_float32_sum_bit_for_bit(d):
    from openscene_amd import ops
    gen = torch.Generator().manual_seed(90 + d)
    r_n = 800
    src = torch.randn(r_n, d, generator=gen) * torch.exp(4 * torch.randn(r_n, 1, generator=gen))     # magnitudes apart: the order shows
    src[3] = 0
    src[4, ::2] = -0.0
    sizes = [1, 2, 0, 65, 700, 1, 0]
    starts = torch.tensor(np.cumsum([0] + sizes), dtype=torch.int64)
    members = torch.randint(0, r_n, (sum(sizes),), generator=gen).int()
    members[0] = 4                                                            # a group of one row of negative zeros: + 0 gives + 0
    got = ops.rows_fold(src.to(dev()), starts.to(dev()), members.to(dev()))
    want = torch.from_numpy(mr.fold(src.numpy(), starts.numpy(), members.numpy()))
    assert got.dtype == torch.float32 and got.shape == (len(sizes), d) and same_bits(got.cpu(), want)
    assert bool((got[2] == 0).all()) and bool((got[6] == 0).all())           # the empty groups
    shuffled = members.clone()
    shuffled[68:768] = members[68:768].flip(0)
    assert not same_bits(ops.rows_fold(src.to(dev()), starts.to(dev()), shuffled.to(dev()))[4].cpu(), want[4])     # the order is the list's
    assert same_bits(ops.rows_fold(src.to(dev()), starts.to(dev()), members.to(dev())), got)


def test_fold_guards():
    from openscene_amd import _lib, ops
    src = torch.ones(5, 16, device=dev())
    starts = torch.tensor([0, 3], device=dev())
    err = torch.zeros(1, dtype=torch.int32, device=dev())
    got = ops.rows_fold(src, starts, i32([0, 5, 1]), err=err)
    assert int(err.item()) == ops.REGIONS_E_REGION and bool((got == 2).all())                           # the bad member skipped
    with pytest.raises(_lib.OpenSceneAmdError, match="region entry"):
        ops.rows_fold(src, starts, i32([0, -1, 1]))
    with pytest.raises(_lib.OpenSceneAmdError, match="region entry"):
        ops.rows_fold(src, torch.tensor([0, 9], device=dev()), i32([0, 1, 2]))                            # starts past the list


# ---------------------------------------------------------------------------------------------------- end to end
def planted_on_device(dtype):
    from openscene_amd.objects import VoxelGrid
    from openscene_amd.search import FeatureBank
    p = rr.planted()
    bank = FeatureBank(rr.PLANT_DIM, dev(), dtype=dtype)
    for i, f in enumerate(p["feats"]):
        bank.add_scene("scene%d" % i, f.to(dev()))
    return p, bank, VoxelGrid.from_scenes([x.to(dev()) for x in p["xyz"]], voxel_size=rr.PLANT_VOXEL)


@pytest.mark.parametrize("dtype", ["fp16", "fp8"])
def test_planted_scenes_end_to_end(dtype):
    from openscene_amd import ops
    from openscene_amd.merge import MergedRegions, merge_regions, region_adjacency, unit_rows
    from openscene_amd.regions import RegionResult, SimilarityGraph
    p, bank, grid = planted_on_device(dtype)
    graph = SimilarityGraph(bank, grid)
    cut = graph.segment(CUT, names=bank.names)
    assert int(torch.bincount(cut.scene.long(), minlength=3).min()) >= 300
    res = merge_regions(bank, grid, cut, similarity=rr.PLANT_SIMILARITY)
    nbr = grid.nbr.cpu().numpy()
    sim64, _ = rr.edges_f64(graph.vox, nbr, 26)
    _, region, r = rr.components(sim64, nbr, rr.PLANT_SIMILARITY, 26)
    assert isinstance(res, MergedRegions) and isinstance(res, RegionResult)
    assert r == res.n_regions == 18 and np.array_equal(res.voxel_region.cpu().numpy(), region)
    assert res.converged and 1 <= res.rounds <= 8 and res.history[-1]["merged"] == 0
    assert torch.equal(res.voxel_region.long(), res.parent[cut.voxel_region.long()])
    rr.assert_records(res, rr.records(region, r, grid.xyz.cpu().numpy(), grid.inverse.cpu().numpy(), grid.coords.cpu().numpy()))
    # the reference loop on the device's sums: the margin condition, the same parents round for round
    lo, hi, c = region_adjacency(grid, cut.voxel_region, cut.n_regions)
    total = cut.descriptors(bank).sum
    want = mr.merge(total.cpu().numpy(), lo.cpu().numpy(), hi.cpu().numpy(), c.cpu().numpy(), rr.PLANT_SIMILARITY)
    assert float(np.abs(want["sims"] - rr.PLANT_SIMILARITY).min()) > rr.PLANT_MARGIN
    assert np.array_equal(want["parent"], res.parent.cpu().numpy()) and want["history"] == res.history
    # the first round alone: the reference's round applied to the device's own sims
    sim = ops.rows_pair_dot(unit_rows(total), lo, hi)
    parent = ops.regions_merge_round(lo, hi, sim, cut.n_regions, rr.PLANT_SIMILARITY)
    first, bits = mr.merge_round(lo.cpu().numpy(), hi.cpu().numpy(), sim.cpu().numpy(), cut.n_regions, rr.PLANT_SIMILARITY)
    assert bits == 0 and parent.cpu().tolist() == first and cut.n_regions - len(set(first)) == res.history[0]["merged"]
    # two calls: identical tensors
    again = merge_regions(bank, grid, cut, similarity=rr.PLANT_SIMILARITY)
    assert torch.equal(again.voxel_region, res.voxel_region) and torch.equal(again.parent, res.parent) and again.history == res.history
    assert all(torch.equal(getattr(again, f), getattr(res, f)) for f in rr.RECORD_FIELDS)
    assert same_bits(again.descriptors(bank).sum, res.descriptors(bank).sum)
    # label and point_labels run on the result
    classes, score = res.label(bank, p["protos"].half().to(dev()))
    assert torch.equal(res.point_labels(classes).cpu(), torch.cat(p["cls"])) and float(score.float().min()) > 0.9


def test_the_strip_and_the_corner_contact():
    from openscene_amd import ops
    from openscene_amd.merge import merge_regions, region_adjacency
    from openscene_amd.objects import VoxelGrid
    from openscene_amd.regions import RegionResult, SimilarityGraph
    from openscene_amd.search import FeatureBank
    feats, xyz = mr.strip()
    bank = FeatureBank(mr.STRIP_DIM, dev())
    bank.add_scene("a", feats.to(dev()))
    grid = VoxelGrid(xyz.to(dev()), None, voxel_size=mr.STRIP_VOXEL)
    graph = SimilarityGraph(bank, grid)
    assert graph.segment(mr.STRIP_SIMILARITY).n_regions == 1                   # single linkage: the chain
    cut = graph.segment(2.0)
    res = merge_regions(bank, grid, cut, similarity=mr.STRIP_SIMILARITY)
    ends = res.point_region.cpu().tolist()
    assert cut.n_regions == mr.STRIP_VOXELS and res.converged and res.n_regions > 1 and ends[0] != ends[-1] and min(ends) >= 0
    lo, hi, c = region_adjacency(grid, cut.voxel_region, cut.n_regions)
    assert lo.shape[0] == mr.STRIP_VOXELS - 1 and bool((c == 1).all())
    one = merge_regions(bank, grid, cut, similarity=mr.STRIP_SIMILARITY, max_rounds=1)
    assert one.rounds == 1 and not one.converged and res.n_regions < one.n_regions < cut.n_regions
    # three cubes: A and B of one prototype touch by one corner voxel pair, C of another meets A face to face
    feats, xyz, cube = mr.corner_cubes()
    bank = FeatureBank(mr.CUBE_DIM, dev())
    bank.add_scene("a", feats.to(dev()))
    grid = VoxelGrid(xyz.to(dev()), None, voxel_size=0.1)
    cube_of_voxel = torch.empty(24, dtype=torch.int64)
    cube_of_voxel[grid.inverse.cpu().long()] = cube
    first = {}
    region = torch.tensor([first.setdefault(int(x), len(first)) for x in cube_of_voxel], dtype=torch.int32).to(dev())
    rec = ops.regions_records(region, 3, grid.xyz, grid.inverse, grid.coords)
    regions = RegionResult(["a"], grid.offsets, grid.voxel_size, 3, region[grid.inverse.long()], region, rec, 0)
    which = {int(cube_of_voxel[v]): int(region[v]) for v in range(24)}
    one = merge_regions(bank, grid, regions, similarity=0.8, min_contact=1)
    assert one.n_regions == 2 and one.rounds == 1 and one.converged
    assert int(one.parent[which[0]]) == int(one.parent[which[1]]) != int(one.parent[which[2]])
    two = merge_regions(bank, grid, regions, similarity=0.8, min_contact=2)
    assert two.n_regions == 3 and two.rounds == 0 and two.converged and torch.equal(two.voxel_region, region)


def test_merge_guards_on_the_device():
    from openscene_amd.merge import merge_regions
    from openscene_amd.objects import VoxelGrid
    from openscene_amd.regions import SimilarityGraph
    p, bank, grid = planted_on_device("fp16")
    graph = SimilarityGraph(bank, grid)
    cut = graph.segment(rr.PLANT_SIMILARITY)
    host = VoxelGrid.__new__(VoxelGrid)                                      # a grid that claims another device
    host.__dict__.update(grid.__dict__)
    host.device = torch.device("cpu")
    with pytest.raises(ValueError, match="device"):
        merge_regions(bank, host, cut)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="finite"):
            merge_regions(bank, grid, cut, similarity=bad)
    with pytest.raises(ValueError, match="min_contact"):
        merge_regions(bank, grid, cut, min_contact=0)
    with pytest.raises(ValueError, match="max_rounds"):
        merge_regions(bank, grid, cut, max_rounds=-1)
    same = merge_regions(bank, grid, cut, similarity=rr.PLANT_SIMILARITY)     # adjacent blobs that do not agree: nothing merges
    assert same.n_regions == 18 and same.rounds == 0 and same.converged and torch.equal(same.voxel_region, cut.voxel_region)
    none = merge_regions(bank, grid, graph.segment(2.0, min_points=100))     # zero regions
    assert none.n_regions == 0 and none.rounds == 0 and none.converged
