"""Host logic of openscene_amd.regions WITHOUT a GPU: the three region ops are replaced by the stand-ins of
tests/regions_reference.py (and those of the search, the objects and the pool by their own), so the argument checks, the
slicing of the voxel rows, the numbering, RegionResult and its conveniences are the code under test.  The reference's own
consistency and the bound constant of tests/test_gpu_regions.py are checked and measured here, on the same inputs."""
import os
import re

import numpy as np
import pytest
import torch

import cpu_backend
import objects_reference as oref
import pool_reference as pr
import regions_reference as rr
import search_contrast_reference as scr
import search_fp8_reference as f8
import search_reference as sr
from openscene_amd import _lib
from openscene_amd import descriptors as D
from openscene_amd import objects as O
from openscene_amd import ops
from openscene_amd import regions as R
from openscene_amd import search as S

CPU = torch.device("cpu")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = {"osn_regions_edges", "osn_regions_label", "osn_regions_records"}


@pytest.fixture(autouse=True)
def cpu_kernels(monkeypatch):
    for name, f in (("coords_unique", oref.coords_unique), ("kmap_build", oref.kmap_build), ("bank_append", sr.bank_append),
                    ("bank_check", sr.bank_check), ("bank_search", scr.bank_search), ("bank_append_fp8", f8.bank_append_fp8),
                    ("bank_search_fp8", scr.bank_search_fp8), ("bank_pool", pr.bank_pool), ("bank_pool_fp8", pr.bank_pool_fp8),
                    ("rows_argmax", cpu_backend.rows_argmax), ("regions_edges", rr.regions_edges),
                    ("regions_label", rr.regions_label), ("regions_records", rr.regions_records)):
        monkeypatch.setattr(ops, name, f)


def planted_bank(dtype="fp16"):
    p = rr.planted()
    bank = S.FeatureBank(rr.PLANT_DIM, CPU, dtype=dtype)
    for i, f in enumerate(p["feats"]):
        bank.add_scene("scene%d" % i, f)
    return p, bank, O.VoxelGrid.from_scenes(p["xyz"], voxel_size=rr.PLANT_VOXEL)


# ---------------------------------------------------------------------------------------------------- the header
def test_the_header_declares_exactly_the_new_entries_the_prototypes_list():
    src = open(os.path.join(ROOT, "include", "openscene_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = {n for n in re.findall(r"\b(osn_[a-z0-9_]+)\s*\(", code) if n.startswith("osn_regions_")}
    assert declared == NEW_ENTRIES == {n for n in _lib.PROTOTYPES if n.startswith("osn_regions_")}
    block = src[src.index("csrc/regions.hip"):src.index("int osn_regions_edges(")]
    for word in ("-inf", "NaN", "k = 4, 10, 12", "smallest voxel row", "integer atomics"):
        assert word in block, word
    for name in NEW_ENTRIES:                                                 # the argument counts agree
        decl = re.search(name + r"\s*\((.*?)\);", code, flags=re.S).group(1)
        assert len(decl.split(",")) == len(_lib.PROTOTYPES[name][1]), name
    assert "regions.hip" in open(os.path.join(ROOT, "openscene_amd", "build.py")).read()


# ---------------------------------------------------------------------------------------------------- the reference itself
def test_self_map_is_its_own_mirror_and_keeps_scenes_apart():
    coords = np.array([(0, 0, 0, 0), (0, 1, 0, 0), (0, 1, 1, 1), (1, 0, 0, 0), (1, 0, 0, 1), (0, 5, 5, 5)], dtype=np.int32)
    nbr = rr.self_map(coords)
    assert nbr[13].tolist() == list(range(6))
    for k in range(27):
        for v in range(6):
            u = nbr[k, v]
            if u >= 0:
                assert nbr[26 - k, u] == v and coords[u, 0] == coords[v, 0]
    assert (nbr[:, 5] >= 0).sum() == 1 and nbr[14, 0] == 1 and nbr[12, 1] == 0 and nbr[4, 4] == 3       # -x = 12, -z = 4
    assert rr.offsets_of(26) == list(range(13)) and rr.offsets_of(6) == [4, 10, 12]


@pytest.mark.parametrize("connectivity", [26, 6])
def test_union_find_and_bfs_agree_and_the_numbering_is_canonical(connectivity):
    case = rr.edge_case("24-special")
    sim, _ = rr.edges_f64(case["vox"], case["nbr"], connectivity)
    gen = torch.Generator().manual_seed(3)
    ppv = torch.randint(1, 5, (sim.shape[1],), generator=gen).numpy()
    fin = sim[np.isfinite(sim)]
    for thr in (-1.0, float(np.median(fin)), float(np.quantile(fin, 0.9)), 2.0):
        for mp in (1, 3):
            a = rr.components(sim, case["nbr"], thr, connectivity, ppv, mp)
            b = rr.components_bfs(sim, case["nbr"], thr, connectivity, ppv, mp)
            root, region, r = a
            assert np.array_equal(root, b[0]) and np.array_equal(region, b[1]) and r == b[2]
            assert bool((root <= np.arange(len(root))).all()) and bool((root[root] == root).all())
            kept = region[region >= 0]
            first = [int(np.nonzero(region == i)[0][0]) for i in range(r)]
            assert sorted(set(kept.tolist())) == list(range(r)) and first == sorted(first)        # ascending smallest rows
            pts = np.bincount(root, weights=ppv, minlength=len(root))
            assert bool(((region >= 0) == (pts[root] >= mp)).all())
    top = rr.components(sim, case["nbr"], 2.0, connectivity)
    assert top[2] == sim.shape[1] and np.array_equal(top[1], np.arange(sim.shape[1]))
    low = rr.components(sim, case["nbr"], -1.0, connectivity)
    assert low[0][case["isolated"]] == case["isolated"] and low[0][case["nan_row"]] == case["nan_row"]     # NaN never unites


def test_the_edge_cases_hold_what_the_gpu_tests_rely_on():
    for name in rr.edge_case_names():
        case = rr.edge_case(name)
        nbr, vox = case["nbr"], case["vox"]
        counts = (np.delete(nbr, 13, 0) >= 0).sum(0)
        assert counts.min() == 0 and counts.max() == 26 and 300 < nbr.shape[1] < 500, name
        assert counts[case["isolated"]] == 0
        sim, bound = rr.edges_f64(vox, nbr, 26)
        assert bool(np.isneginf(sim[:, case["isolated"]]).all())
        if case["nan_row"] is None:
            assert not np.isnan(sim).any()
            continue
        bits = vox.view(torch.int16).long() & 0x7FFF
        assert int(((bits > 0) & (bits < 0x0400)).sum()) > 20, name           # fp16 subnormals are there
        n, z = case["nan_row"], case["zero_row"]
        touches_nan = (nbr[:13] == n) | (np.arange(nbr.shape[1]) == n)[None, :]
        assert np.array_equal(np.isnan(sim), touches_nan & (nbr[:13] >= 0)) and np.isnan(sim).sum() > 0
        touches_zero = ((nbr[:13] == z) | (np.arange(nbr.shape[1]) == z)[None, :]) & (nbr[:13] >= 0) & ~np.isnan(sim)
        assert touches_zero.sum() > 0 and bool((sim[touches_zero] == 0).all())


# ---------------------------------------------------------------------------------------------------- the bound constant
def test_the_bound_constant_is_four_times_the_sequential_sums_worst_ratio():
    worst, worst_name = 0.0, None
    for name in rr.edge_case_names():
        case = rr.edge_case(name)
        for conn in (26, 6):
            want, bound = rr.edges_f64(case["vox"], case["nbr"], conn)
            got = rr.edges_f32(case["vox"], case["nbr"], conn)
            ratio, bad, odd = rr.sim_errors(got, want, bound, rr.SIM_C_CAP)
            assert bad == 0 and odd == 0, (name, conn)
            print("%-12s conn %2d  error / abs-sum %.3e" % (name, conn, ratio))
            if ratio > worst:
                worst, worst_name = ratio, "%s/%d" % (name, conn)
    print("worst: %s %.4e; recorded %.3e; SIM_C %.3e; cap %.3e" % (worst_name, worst, rr.SIM_MEASURED_RATIO, rr.SIM_C, rr.SIM_C_CAP))
    assert worst <= rr.SIM_MEASURED_RATIO <= 1.01 * worst, (worst_name, worst)
    assert rr.SIM_C == 4 * rr.SIM_MEASURED_RATIO and rr.SIM_C <= rr.SIM_C_CAP == 1023 * 2.0 ** -24


# ---------------------------------------------------------------------------------------------------- planted scenes
def test_the_planted_scenes_keep_their_distance_from_the_threshold():
    """The float64 reference on the inputs as the generator makes them: no sim within PLANT_MARGIN of the threshold (asserted by
    planted_check), 18 pure regions, for both bank kinds; the margin is more than 16 x SIM_C_CAP."""
    assert rr.PLANT_MARGIN > 16 * rr.SIM_C_CAP
    for dtype in ("fp16", "fp8"):
        p, bank, grid = planted_bank(dtype)
        graph = R.SimilarityGraph(bank, grid)
        res = graph.segment(rr.PLANT_SIMILARITY)
        classes = rr.planted_check(graph, res, p["cls"])
        assert sorted(classes.reshape(3, 6).tolist()[0]) == list(range(6))
        assert res.n_voxels.tolist() == [rr.PLANT_SIDE ** 3] * 18 and res.n_dropped_points == 0


@pytest.mark.parametrize("dtype", ["fp16", "fp8"])
def test_regions_end_to_end_through_the_stand_ins(dtype):
    p, bank, grid = planted_bank(dtype)
    graph = R.SimilarityGraph(bank, grid, slice_voxels=100)                    # four slices, the last one short
    whole = R.SimilarityGraph(bank, grid)
    assert torch.equal(graph.vox.view(torch.int16), whole.vox.view(torch.int16))          # slicing changes no bit
    assert graph.vox.dtype == torch.float16 and graph.sim.shape == (13, grid.n_voxels) and graph.sim.dtype == torch.float32
    res = graph.segment(rr.PLANT_SIMILARITY, names=bank.names)
    planted_cls = rr.planted_check(graph, res, p["cls"])
    assert res.point_region.dtype == torch.int32 and res.voxel_region.dtype == torch.int32
    want = rr.records(res.voxel_region.numpy(), res.n_regions, grid.xyz.numpy(), grid.inverse.numpy(), grid.coords.numpy())
    rr.assert_records(res, want)
    assert torch.equal(res.centroid, (res.vox_sum.double() / res.n_points.double()[:, None] + 0.5) * rr.PLANT_VOXEL)
    # regions(): one scene's, largest first, ties by id
    listed = res.regions("scene1")
    assert [r["id"] for r in listed] == list(range(6, 12)) and listed == res.regions(1)
    assert all(r["n_points"] == rr.PLANT_SIDE ** 3 * rr.PLANT_POINTS and r["n_voxels"] == 64 for r in listed)
    assert all(len(r["centroid"]) == 3 and r["box_min"][0] <= r["centroid"][0] <= r["box_max"][0] for r in listed)
    # groups / descriptors / label / point_labels
    g = res.groups()
    assert g.n_groups == 18 and g.n_entries == grid.n_points
    assert torch.equal(g.rows[g.starts[3]:g.starts[4]], torch.nonzero(res.point_region == 3).reshape(-1))
    desc = res.descriptors(bank)
    assert torch.equal(desc.count, res.n_points) and desc.mean.shape == (18, rr.PLANT_DIM)
    text = p["protos"].half()
    classes, score = res.label(bank, text)
    assert classes.dtype == torch.int64 and score.dtype == torch.float16 and torch.equal(classes, planted_cls)
    assert float(score.float().min()) > 0.9
    heat = S.heat_map(desc.mean, text)
    assert torch.equal(score, heat.max(1)[0])
    rel_cls, rel = res.label(bank, text[:3], negatives=text[3:], temperature=0.05)
    own = planted_cls < 3
    assert torch.equal(rel_cls[own], planted_cls[own]) and float(rel[own].float().min()) > 0.9 and float(rel[~own].float().max()) < 0.1
    labels = res.point_labels(classes)
    assert labels.dtype == torch.int64 and torch.equal(labels, torch.cat(p["cls"]))
    # a region as the next query finds its own points
    q = desc.queries()[7:8]
    hits = S.search(bank, q, thresholds=0.8, return_heat=True).heat[:, 0].float() >= 0.8
    assert torch.equal(hits, torch.cat(p["cls"]) == int(planted_cls[7]))
    # the package-level form
    import openscene_amd
    again = openscene_amd.segment(bank, grid, similarity=rr.PLANT_SIMILARITY)
    assert again.names == bank.names and torch.equal(again.point_region, res.point_region)


def test_segment_reuses_sim_and_min_points_renumbers():
    p, bank, grid = planted_bank()
    graph = R.SimilarityGraph(bank, grid)
    sim, bits = graph.sim, graph.sim.clone()
    top = graph.segment(2.0)                                                 # above every sim: one region per voxel, in voxel order
    assert top.n_regions == grid.n_voxels and torch.equal(top.voxel_region, torch.arange(grid.n_voxels, dtype=torch.int32))
    ppv = torch.bincount(grid.inverse.long(), minlength=grid.n_voxels)
    assert torch.equal(top.n_points, ppv) and graph.sim is sim and torch.equal(graph.sim, bits)
    # make one blob's voxels single by raising the threshold over its sims only: use min_points on the per-voxel regions
    few = graph.segment(2.0, min_points=int(ppv.max()) + 1)
    assert few.n_regions == 0 and few.n_dropped_points == grid.n_points and bool((few.point_region == -1).all())
    assert few.label(bank, p["protos"].half())[0].shape == (0,) and few.regions(0) == []
    _, region, r = rr.components(graph.sim.numpy(), grid.nbr.numpy(), 0.97, 26, ppv.numpy(), 3)
    some = graph.segment(0.97, min_points=3)                                 # (whatever 0.97 cuts: the reference decides)
    assert some.n_regions == r and np.array_equal(some.voxel_region.numpy(), region)
    assert some.n_dropped_points == int((some.point_region == -1).sum()) == grid.n_points - int(some.n_points.sum())
    labels = some.point_labels(torch.arange(r))
    assert torch.equal(labels, some.point_region.long())


# ---------------------------------------------------------------------------------------------------- arguments
def test_argument_errors():
    p, bank, grid = planted_bank()
    with pytest.raises(TypeError):
        R.SimilarityGraph(bank.features, grid)
    with pytest.raises(TypeError):
        R.SimilarityGraph(bank, grid.coords)
    short = S.FeatureBank(rr.PLANT_DIM, CPU)
    short.add_scene("a", p["feats"][0])
    with pytest.raises(ValueError, match="rows"):
        R.SimilarityGraph(short, grid)
    with pytest.raises(ValueError):
        R.SimilarityGraph(bank, grid, slice_voxels=0)
    graph = R.SimilarityGraph(bank, grid)
    for bad in (float("nan"), float("inf"), float("-inf")):
        with pytest.raises(ValueError, match="finite"):
            graph.segment(bad)
    with pytest.raises(ValueError):
        graph.segment(0.5, min_points=0)
    with pytest.raises(ValueError):
        graph.segment(0.5, names=["a"])
    res = graph.segment(rr.PLANT_SIMILARITY)
    with pytest.raises(ValueError):
        res.point_labels(torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError):
        res.point_labels(torch.zeros(18))
    with pytest.raises(IndexError):
        res.regions(5)
    assert ops.regions_n_off(26) == 13 and ops.regions_n_off(6) == 3
    with pytest.raises(ValueError):
        ops.regions_n_off(18)
    err = torch.tensor([5], dtype=torch.int32)
    with pytest.raises(_lib.OpenSceneAmdError, match="neighbour"):
        ops.regions_check(err)
    assert int(err) == 0
    ops.regions_check(err)
