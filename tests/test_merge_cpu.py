"""Host logic of openscene_amd.merge WITHOUT a GPU: the four merge ops are replaced by the stand-ins of
tests/merge_reference.py (and the region, search, objects and pool ops by their own), so the argument checks, the loop, the
numbering, the contraction of the pair list and MergedRegions are the code under test.  The claims the merge rule is chosen
for -- rounds, the strip, the corner contact -- are checked on the reference itself."""
import os
import re

import numpy as np
import pytest
import torch

import cpu_backend
import merge_reference as mr
import objects_reference as oref
import pool_reference as pr
import regions_reference as rr
import search_contrast_reference as scr
import search_fp8_reference as f8
import search_reference as sr
from openscene_amd import _lib
from openscene_amd import merge as M
from openscene_amd import objects as O
from openscene_amd import ops
from openscene_amd import regions as R
from openscene_amd import search as S

CPU = torch.device("cpu")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = {"osn_merge_contacts", "osn_rows_pair_dot", "osn_merge_round", "osn_merge_ws_bytes", "osn_rows_fold"}
CUT = 0.995                      # the over-segmentation of the planted scenes: same-blob voxel sims start at 0.96


@pytest.fixture(autouse=True)
def cpu_kernels(monkeypatch):
    for name, f in (("coords_unique", oref.coords_unique), ("kmap_build", oref.kmap_build), ("bank_append", sr.bank_append),
                    ("bank_check", sr.bank_check), ("bank_search", scr.bank_search), ("bank_append_fp8", f8.bank_append_fp8),
                    ("bank_search_fp8", scr.bank_search_fp8), ("bank_pool", pr.bank_pool), ("bank_pool_fp8", pr.bank_pool_fp8),
                    ("rows_argmax", cpu_backend.rows_argmax), ("regions_edges", rr.regions_edges),
                    ("regions_label", rr.regions_label), ("regions_records", rr.regions_records),
                    ("regions_contacts", mr.regions_contacts), ("rows_pair_dot", mr.rows_pair_dot),
                    ("regions_merge_round", mr.regions_merge_round), ("rows_fold", mr.rows_fold)):
        monkeypatch.setattr(ops, name, f)


def planted_bank(dtype="fp16"):
    p = rr.planted()
    bank = S.FeatureBank(rr.PLANT_DIM, CPU, dtype=dtype)
    for i, f in enumerate(p["feats"]):
        bank.add_scene("scene%d" % i, f)
    return p, bank, O.VoxelGrid.from_scenes(p["xyz"], voxel_size=rr.PLANT_VOXEL)


def one_scene(feats, xyz, voxel_size, dim):
    bank = S.FeatureBank(dim, CPU)
    bank.add_scene("a", feats)
    return bank, O.VoxelGrid(xyz, None, voxel_size=voxel_size)


def result_from_labels(grid, label_of_voxel):
    """A RegionResult of a hand-made labelling (any integers >= 0 per voxel), numbered canonically."""
    first = {}
    region = torch.tensor([first.setdefault(int(x), len(first)) for x in label_of_voxel], dtype=torch.int32)
    rec = ops.regions_records(region, len(first), grid.xyz, grid.inverse, grid.coords)
    return R.RegionResult(["a"], grid.offsets, grid.voxel_size, len(first), region[grid.inverse.long()], region, rec, 0)


# ---------------------------------------------------------------------------------------------------- the header
def test_the_header_declares_exactly_the_new_entries_the_prototypes_list():
    src = open(os.path.join(ROOT, "include", "openscene_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    block = code[code.index("int osn_merge_contacts("):code.index("osn_voxelize_ws_bytes")]
    declared = set(re.findall(r"\b(osn_[a-z0-9_]+)\s*\(", block))
    assert declared == NEW_ENTRIES and NEW_ENTRIES <= set(_lib.PROTOTYPES)
    assert {n for n in _lib.PROTOTYPES if n.startswith("osn_merge_")} == {n for n in NEW_ENTRIES if n.startswith("osn_merge_")}
    text = src[src.index("csrc/merge.hip"):src.index("int osn_merge_contacts(")]
    for word in ("-inf", "NaN", "-0 orders below +0", "mutual", "0xFFFFFFFF - e", "csrc/rowdot.h", "same bits", "no atomics",
                 "smallest group member", "8 = a pair end outside"):
        assert word in text.replace("No atomics", "no atomics"), word
    for name in NEW_ENTRIES:                                                 # the argument counts agree
        decl = re.search(name + r"\s*\((.*?)\);", code, flags=re.S).group(1)
        assert len(decl.split(",")) == len(_lib.PROTOTYPES[name][1]), name
    assert "merge.hip" in open(os.path.join(ROOT, "openscene_amd", "build.py")).read()
    assert ops.REGIONS_E_PAIR == mr.E_PAIR == 8 and (ops.REGIONS_E_NBR, ops.REGIONS_E_INVERSE, ops.REGIONS_E_REGION) == (1, 2, 4)
    edges = open(os.path.join(ROOT, "openscene_amd", "csrc", "regions.hip")).read()
    merge = open(os.path.join(ROOT, "openscene_amd", "csrc", "merge.hip")).read()
    for unit in (edges, merge):                                              # one shared body, no second copy of the sum
        assert '#include "rowdot.h"' in unit and "row_dot<NV>(" in unit and "__shfl_xor(acc" not in unit


# ---------------------------------------------------------------------------------------------------- the reference itself
def test_the_order_key_orders_like_the_float_and_the_round_breaks_ties_by_edge_index():
    vals = [float("-inf"), -2.5, -1e-40, -0.0, 0.0, 1e-40, 0.5, 1.0, float("inf")]
    keys = [mr.order_key(v) for v in vals]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)               # (-0 below +0)
    # a - b and b - c tie: the lower edge index (a, b) wins from both ends, c points at a mutual pair and joins
    parent, bits = mr.merge_round([0, 1], [1, 2], [0.9, 0.9], 3, 0.5)
    assert parent == [0, 0, 0] and bits == 0
    assert mr.merge_round([0, 1], [1, 2], [0.9, 0.9], 3, 0.5, rule="mutual")[0] == [0, 0, 2]
    # a chain a -> b -> c -> d with (c, d) mutual: b joins, a does not; "tree" takes the whole chain
    lo, hi, sim = [0, 1, 2], [1, 2, 3], [0.6, 0.7, 0.8]
    assert mr.merge_round(lo, hi, sim, 4, 0.5)[0] == [0, 1, 1, 1]
    assert mr.merge_round(lo, hi, sim, 4, 0.5, rule="tree")[0] == [0, 0, 0, 0]
    assert mr.merge_round(lo, hi, sim, 4, 0.5, rule="mutual")[0] == [0, 1, 2, 2]
    # the threshold: equal passes, NaN and -inf never do; a bad end is skipped and reported
    parent, bits = mr.merge_round([0, 2, 4, 6, 7], [1, 3, 5, 7, 9], [0.5, np.nextafter(np.float32(0.5), np.float32(0)), float("nan"),
                                                                   float("-inf"), 0.9], 9, 0.5)
    assert parent == list(range(1)) + [0] + list(range(2, 9)) and bits == mr.E_PAIR


def test_contacts_and_fold_of_the_reference_by_hand():
    coords = np.array([(0, 0, 0, 0), (0, 1, 0, 0), (0, 2, 0, 0), (0, 1, 1, 0), (1, 0, 0, 0), (1, 1, 0, 0)], dtype=np.int32)
    nbr = rr.self_map(coords)
    lo, hi, c = mr.adjacency([0, 1, 1, 0, 2, 3], nbr, 26, 4)                 # scene 1 never touches scene 0
    assert list(zip(lo.tolist(), hi.tolist(), c.tolist())) == [(0, 1, 3), (2, 3, 1)]       # voxels 0-1, 1-3 and the diagonal 2-3
    lo, hi, c = mr.adjacency([0, 1, 1, 0, 2, 3], nbr, 6, 4)                  # faces only: 0-1 and 1-3, not the diagonal
    assert list(zip(lo.tolist(), hi.tolist(), c.tolist())) == [(0, 1, 2), (2, 3, 1)]
    lo, hi, c = mr.adjacency([0, -1, 1, 0, 2, 2], nbr, 26, 3)                # -1 touches nothing; one region has no contact
    assert list(zip(lo.tolist(), hi.tolist(), c.tolist())) == [(0, 1, 1)]
    assert mr.contact_keys([0, 5, 1, 0, 2, 2], nbr, 26, 3)[1] == mr.E_REGION
    src = np.array([[1e8] * 8, [1.0] * 8, [-1e8] * 8, [3.0] * 8], dtype=np.float32)
    out = mr.fold(src, [0, 3, 3, 4], [0, 1, 2, 3])
    assert out[0].tolist() == [0.0] * 8 and out[1].tolist() == [0.0] * 8 and out[2].tolist() == [3.0] * 8    # (1e8 + 1) - 1e8 = 0 in float32
    assert mr.fold(src, [0, 3], [1, 0, 2])[0].tolist() == [0.0] * 8 and mr.fold(src, [0, 3], [0, 2, 1])[0].tolist() == [1.0] * 8


# ---------------------------------------------------------------------------------------------------- planted scenes
@pytest.mark.parametrize("dtype", ["fp16", "fp8"])
def test_the_planted_scenes_merge_back_to_the_planted_partition(dtype):
    p, bank, grid = planted_bank(dtype)
    graph = R.SimilarityGraph(bank, grid)
    cut = graph.segment(CUT, names=bank.names)
    per_scene = torch.bincount(cut.scene.long(), minlength=3)
    assert int(per_scene.min()) >= 300, per_scene
    res = M.merge_regions(bank, grid, cut, similarity=rr.PLANT_SIMILARITY)
    # the float64 reference: components of the voxel sims at PLANT_SIMILARITY = the 18 planted blobs, canonical numbering
    nbr = grid.nbr.numpy()
    sim64, _ = rr.edges_f64(graph.vox, nbr, 26)
    _, region, r = rr.components(sim64, nbr, rr.PLANT_SIMILARITY, 26)
    assert r == res.n_regions == 3 * rr.PLANT_PROTOTYPES and np.array_equal(res.voxel_region.numpy(), region)
    assert isinstance(res, R.RegionResult) and res.converged and 1 <= res.rounds <= 8
    assert res.parent.dtype == torch.int64 and res.parent.shape == (cut.n_regions,)
    assert torch.equal(res.voxel_region.long(), res.parent[cut.voxel_region.long()])           # consistent with both partitions
    assert torch.equal(res.point_region, res.voxel_region[grid.inverse.long()]) and res.point_region.dtype == torch.int32
    assert res.names == bank.names and res.offsets == cut.offsets and res.n_dropped_points == 0
    assert [h["regions"] for h in res.history][0] == cut.n_regions and res.history[-1]["merged"] == 0
    assert sum(h["merged"] for h in res.history) == cut.n_regions - 18 and sum(h["merged"] > 0 for h in res.history) == res.rounds
    rr.assert_records(res, rr.records(region, r, grid.xyz.numpy(), grid.inverse.numpy(), grid.coords.numpy()))
    # the reference loop on the same sums and its own adjacency: float64 sims, every one far from the threshold
    lo, hi, c = mr.adjacency(cut.voxel_region.numpy(), nbr, 26, cut.n_regions)
    glo, ghi, gc = M.region_adjacency(grid, cut.voxel_region, cut.n_regions)
    assert np.array_equal(glo.numpy(), lo) and np.array_equal(ghi.numpy(), hi) and np.array_equal(gc.numpy(), c)
    assert glo.dtype == torch.int32 and gc.dtype == torch.int64
    total = cut.descriptors(bank).sum.numpy()
    want = mr.merge(total, lo, hi, c, rr.PLANT_SIMILARITY)
    assert len(want["sims"]) > 0 and float(np.abs(want["sims"] - rr.PLANT_SIMILARITY).min()) > rr.PLANT_MARGIN      # the margin condition
    assert np.array_equal(want["parent"], res.parent.numpy()) and want["rounds"] == res.rounds and want["converged"]
    assert want["history"] == res.history
    # inherited conveniences work unchanged
    classes, score = res.label(bank, p["protos"].half())
    assert torch.equal(res.point_labels(classes), torch.cat(p["cls"])) and float(score.float().min()) > 0.9
    assert res.groups().n_groups == 18 and torch.equal(res.descriptors(bank).count, res.n_points)
    assert len(res.regions("scene1")) == 6
    import openscene_amd
    again = openscene_amd.merge_regions(bank, grid, cut, similarity=rr.PLANT_SIMILARITY)
    assert torch.equal(again.voxel_region, res.voxel_region) and torch.equal(again.parent, res.parent)


def test_the_star_needs_a_handful_of_rounds_where_mutual_pairs_need_dozens():
    """The documented reason for the rule, on the reference: a property, not a tolerance."""
    p, bank, grid = planted_bank()
    cut = R.SimilarityGraph(bank, grid).segment(CUT)
    nbr = grid.nbr.numpy()
    lo, hi, c = mr.adjacency(cut.voxel_region.numpy(), nbr, 26, cut.n_regions)
    total = cut.descriptors(bank).sum.numpy()
    star = mr.merge(total, lo, hi, c, rr.PLANT_SIMILARITY, rule="star")
    mutual = mr.merge(total, lo, hi, c, rr.PLANT_SIMILARITY, rule="mutual", max_rounds=200)
    print("star %d rounds, mutual-only %d rounds" % (star["rounds"], mutual["rounds"]))
    assert star["converged"] and mutual["converged"] and star["n_regions"] == mutual["n_regions"] == 18
    assert np.array_equal(star["parent"], mutual["parent"])
    assert star["rounds"] <= 8 and mutual["rounds"] > 30


# ---------------------------------------------------------------------------------------------------- the strip
def test_the_strip_single_linkage_joins_the_ends_and_the_merge_does_not():
    feats, xyz = mr.strip()
    bank, grid = one_scene(feats, xyz, mr.STRIP_VOXEL, mr.STRIP_DIM)
    graph = R.SimilarityGraph(bank, grid)
    assert graph.segment(mr.STRIP_SIMILARITY).n_regions == 1                   # the chain
    cut = graph.segment(2.0)                                                 # one region per voxel
    assert cut.n_regions == mr.STRIP_VOXELS
    res = M.merge_regions(bank, grid, cut, similarity=mr.STRIP_SIMILARITY)
    assert res.converged and res.n_regions > 1
    pr_ = res.point_region.tolist()
    assert pr_[0] != pr_[-1] and pr_[0] >= 0 and pr_[-1] >= 0                # the two end voxels (points 0 and 59)
    x = grid.coords[:, 1].long()
    order = torch.sort(x)[1]
    along = res.voxel_region[order].tolist()
    assert along == sorted(along) or along == sorted(along, reverse=True) or len(set(along)) == res.n_regions     # runs along the strip
    want = mr.merge(cut.descriptors(bank).sum.numpy(), *mr.adjacency(cut.voxel_region.numpy(), grid.nbr.numpy(), 26, cut.n_regions),
                    mr.STRIP_SIMILARITY, sims="f32")
    assert np.array_equal(want["parent"], res.parent.numpy()) and want["rounds"] == res.rounds
    tree = mr.merge(cut.descriptors(bank).sum.numpy(), *mr.adjacency(cut.voxel_region.numpy(), grid.nbr.numpy(), 26, cut.n_regions),
                    mr.STRIP_SIMILARITY, rule="tree")
    print("strip: star %d regions in %d rounds; tree %d regions" % (res.n_regions, res.rounds, tree["n_regions"]))
    # max_rounds: one round only, not converged; zero rounds: the input partition
    one = M.merge_regions(bank, grid, cut, similarity=mr.STRIP_SIMILARITY, max_rounds=1)
    assert one.rounds == 1 and not one.converged and res.n_regions < one.n_regions < cut.n_regions and len(one.history) == 1
    none = M.merge_regions(bank, grid, cut, similarity=mr.STRIP_SIMILARITY, max_rounds=0)
    assert none.rounds == 0 and not none.converged and torch.equal(none.voxel_region, cut.voxel_region) and none.history == []
    assert torch.equal(none.parent, torch.arange(cut.n_regions))


# ---------------------------------------------------------------------------------------------------- min_contact
def test_min_contact_keeps_a_corner_contact_apart():
    feats, xyz, cube = mr.corner_cubes()
    bank, grid = one_scene(feats, xyz, 0.1, mr.CUBE_DIM)
    assert grid.n_voxels == 24
    cube_of_voxel = torch.empty(24, dtype=torch.int64)
    cube_of_voxel[grid.inverse.long()] = cube
    regions = result_from_labels(grid, cube_of_voxel.tolist())
    which = {int(cube_of_voxel[v]): int(regions.voxel_region[v]) for v in range(24)}        # cube -> region id
    lo, hi, c = M.region_adjacency(grid, regions.voxel_region, 3)
    contact = {(int(a), int(b)): int(n) for a, b, n in zip(lo, hi, c)}
    ab, ac = tuple(sorted((which[0], which[1]))), tuple(sorted((which[0], which[2])))
    assert contact[ab] == 1 and contact[ac] >= 4 and len(contact) == 2
    one = M.merge_regions(bank, grid, regions, similarity=0.8, min_contact=1)
    assert one.n_regions == 2 and one.parent[which[0]] == one.parent[which[1]] != one.parent[which[2]] and one.converged
    assert one.rounds == 1 and int(one.n_voxels.max()) == 16
    two = M.merge_regions(bank, grid, regions, similarity=0.8, min_contact=2)
    assert two.n_regions == 3 and two.rounds == 0 and two.converged and torch.equal(two.voxel_region, regions.voxel_region)
    assert [h["pairs"] for h in two.history] == [1] and [h["pairs"] for h in one.history][0] == 2


# ---------------------------------------------------------------------------------------------------- edges of the loop
def test_nothing_to_merge_returns_the_input_partition():
    p, bank, grid = planted_bank()
    graph = R.SimilarityGraph(bank, grid)
    none = graph.segment(2.0, min_points=100)                                # zero regions
    res = M.merge_regions(bank, grid, none)
    assert res.n_regions == 0 and res.rounds == 0 and res.converged and res.parent.shape == (0,) and res.history == []
    assert bool((res.voxel_region == -1).all()) and res.n_dropped_points == grid.n_points
    whole = graph.segment(-1.0)                                              # one region per scene: scenes never touch
    res = M.merge_regions(bank, grid, whole, similarity=-1.0)
    assert res.n_regions == 3 and res.rounds == 0 and res.converged and torch.equal(res.voxel_region, whole.voxel_region)
    planted = graph.segment(rr.PLANT_SIMILARITY)                             # adjacent, but nothing agrees: a round that merges nothing
    res = M.merge_regions(bank, grid, planted, similarity=rr.PLANT_SIMILARITY)
    assert res.n_regions == 18 and res.rounds == 0 and res.converged and len(res.history) == 1 and res.history[0]["merged"] == 0
    # regions dropped by min_points stay dropped and touch nothing
    few = graph.segment(CUT, min_points=rr.PLANT_POINTS + 1)
    if few.n_regions:
        res = M.merge_regions(bank, grid, few, similarity=rr.PLANT_SIMILARITY)
        assert torch.equal(res.voxel_region == -1, few.voxel_region == -1) and res.n_dropped_points == few.n_dropped_points


# ---------------------------------------------------------------------------------------------------- arguments
def test_argument_errors_of_merge_regions():
    p, bank, grid = planted_bank()
    cut = R.SimilarityGraph(bank, grid).segment(rr.PLANT_SIMILARITY)
    with pytest.raises(TypeError):
        M.merge_regions(bank.features, grid, cut)
    with pytest.raises(TypeError):
        M.merge_regions(bank, grid.coords, cut)
    with pytest.raises(TypeError):
        M.merge_regions(bank, grid, cut.voxel_region)
    short = S.FeatureBank(rr.PLANT_DIM, CPU)
    short.add_scene("a", p["feats"][0])
    with pytest.raises(ValueError, match="rows"):
        M.merge_regions(short, grid, cut)
    other = O.VoxelGrid(p["xyz"][0], None, voxel_size=rr.PLANT_VOXEL)
    with pytest.raises(ValueError, match="rows"):
        M.merge_regions(bank, other, cut)
    small = O.VoxelGrid(torch.cat(p["xyz"]), None, voxel_size=4 * rr.PLANT_VOXEL)          # the same points, other voxels
    with pytest.raises(ValueError, match="voxels"):
        M.merge_regions(bank, small, cut)
    host = O.VoxelGrid.__new__(O.VoxelGrid)                                  # a grid that claims another device
    host.__dict__.update(grid.__dict__)
    host.device = torch.device("meta")
    with pytest.raises(ValueError, match="device"):
        M.merge_regions(bank, host, cut)
    for bad in (float("nan"), float("inf"), float("-inf")):
        with pytest.raises(ValueError, match="finite"):
            M.merge_regions(bank, grid, cut, similarity=bad)
    with pytest.raises(ValueError, match="min_contact"):
        M.merge_regions(bank, grid, cut, min_contact=0)
    with pytest.raises(ValueError, match="max_rounds"):
        M.merge_regions(bank, grid, cut, max_rounds=-1)
    with pytest.raises(TypeError):
        M.region_adjacency(grid, cut.voxel_region.long(), cut.n_regions)
    with pytest.raises(TypeError):
        M.region_adjacency(grid.nbr, cut.voxel_region, cut.n_regions)
    with pytest.raises(ValueError, match="voxels"):
        M.region_adjacency(grid, cut.voxel_region[:-1], cut.n_regions)


def test_argument_errors_of_the_wrappers(monkeypatch):
    monkeypatch.undo()                                                        # the real wrappers: every check comes before the library is touched
    monkeypatch.setattr(ops, "_prep", lambda dev: None)
    i32 = lambda *a: torch.tensor(a, dtype=torch.int32)                      # noqa: E731
    nbr = torch.full((27, 4), -1, dtype=torch.int32)
    region = i32(0, 0, 1, 1)
    with pytest.raises(TypeError):
        ops.regions_contacts(region.long(), nbr, 26, 2)
    with pytest.raises(ValueError):
        ops.regions_contacts(region.reshape(2, 2), nbr, 26, 2)
    with pytest.raises(ValueError, match="connectivity"):
        ops.regions_contacts(region, nbr, 18, 2)
    with pytest.raises(ValueError, match="nbr"):
        ops.regions_contacts(region, nbr[:, :3], 26, 2)
    with pytest.raises(ValueError, match="n_regions"):
        ops.regions_contacts(region, nbr, 26, 5)
    with pytest.raises(ValueError, match="err"):
        ops.regions_contacts(region, nbr, 26, 2, err=torch.zeros(2, dtype=torch.int32))
    rows = torch.zeros((3, 16), dtype=torch.float16)
    with pytest.raises(TypeError):
        ops.rows_pair_dot(rows.float(), i32(0), i32(1))
    with pytest.raises(ValueError, match="multiple of 8"):
        ops.rows_pair_dot(torch.zeros((3, 12), dtype=torch.float16), i32(0), i32(1))
    with pytest.raises(ValueError, match="1024"):
        ops.rows_pair_dot(torch.zeros((3, 1032), dtype=torch.float16), i32(0), i32(1))
    with pytest.raises(ValueError):
        ops.rows_pair_dot(rows[:, ::2], i32(0), i32(1))
    with pytest.raises(TypeError):
        ops.rows_pair_dot(rows, torch.tensor([0]), i32(1))
    with pytest.raises(ValueError, match="one length"):
        ops.rows_pair_dot(rows, i32(0, 1), i32(1))
    sim = torch.zeros(2)
    with pytest.raises(TypeError):
        ops.regions_merge_round(i32(0, 1), i32(1, 2), sim.double(), 3, 0.5)
    with pytest.raises(TypeError):
        ops.regions_merge_round(i32(0, 1).long(), i32(1, 2), sim, 3, 0.5)
    with pytest.raises(ValueError, match="one per pair"):
        ops.regions_merge_round(i32(0, 1), i32(1, 2), torch.zeros(3), 3, 0.5)
    with pytest.raises(ValueError, match="n_regions"):
        ops.regions_merge_round(i32(0, 1), i32(1, 2), sim, -1, 0.5)
    with pytest.raises(ValueError, match="n_regions"):
        ops.regions_merge_round(i32(0, 1), i32(1, 2), sim, 2 ** 31, 0.5)
    for bad in (float("nan"), float("inf"), float("-inf")):
        with pytest.raises(ValueError, match="finite"):
            ops.regions_merge_round(i32(0, 1), i32(1, 2), sim, 3, bad)
    src = torch.zeros((3, 16))
    starts = torch.tensor([0, 2])
    with pytest.raises(TypeError):
        ops.rows_fold(src.half(), starts, i32(0, 1))
    with pytest.raises(ValueError, match="multiple of 8"):
        ops.rows_fold(torch.zeros((3, 12)), starts, i32(0, 1))
    with pytest.raises(ValueError, match="1024"):
        ops.rows_fold(torch.zeros((3, 1032)), starts, i32(0, 1))
    with pytest.raises(ValueError, match="starts"):
        ops.rows_fold(src, starts.int(), i32(0, 1))
    with pytest.raises(ValueError, match="starts"):
        ops.rows_fold(src, torch.empty(0, dtype=torch.int64), i32(0, 1))
    with pytest.raises(ValueError, match="members"):
        ops.rows_fold(src, starts, torch.tensor([0, 1]))
    err = torch.tensor([8], dtype=torch.int32)
    with pytest.raises(_lib.OpenSceneAmdError, match="pair end"):
        ops.regions_check(err)
    assert int(err) == 0
