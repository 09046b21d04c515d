"""Host logic of openscene_amd.objects WITHOUT a GPU: the kernels (ops.coords_unique, ops.kmap_build, ops.objects_find) are
replaced by the stand-ins of tests/objects_reference.py; the grid's bookkeeping, the argument checks, the derived
fields, ObjectResult.objects / rank_scenes and the SearchResult forwarder are the code under test."""
import numpy as np
import pytest
import torch

import objects_reference as oref
import search_reference as sr
from openscene_amd import objects as O
from openscene_amd import ops
from openscene_amd import search as S

CPU = torch.device("cpu")
VS = 0.5


@pytest.fixture(autouse=True)
def cpu_kernels(monkeypatch):
    monkeypatch.setattr(ops, "coords_unique", oref.coords_unique)
    monkeypatch.setattr(ops, "kmap_build", oref.kmap_build)
    monkeypatch.setattr(ops, "objects_find", oref.objects_find)
    monkeypatch.setattr(ops, "bank_append", sr.bank_append)
    monkeypatch.setattr(ops, "bank_check", sr.bank_check)
    monkeypatch.setattr(ops, "bank_search", sr.bank_search)


def centres(cells):
    return (torch.tensor(cells, dtype=torch.float64) + 0.5) * VS


def test_grid_bookkeeping_one_scene():
    xyz = centres([[0, 0, 0], [0, 0, 0], [1, 0, 0], [-1, -1, -1], [5, 5, 5]])
    g = O.VoxelGrid(xyz, voxel_size=VS)
    assert g.n_points == 5 and g.n_voxels == 4 and g.n_scenes == 1 and g.offsets == [0, 5]
    assert g.coords.tolist() == [[0, 0, 0, 0], [0, 1, 0, 0], [0, -1, -1, -1], [0, 5, 5, 5]]
    assert g.inverse.tolist() == [0, 0, 1, 2, 3] and g.inverse.dtype == torch.int32
    assert g.xyz.dtype == torch.float32 and g.nbr.shape == (27, 4)
    assert g.nbr[13].tolist() == [0, 1, 2, 3]
    assert g.nbr[14].tolist() == [1, -1, -1, -1] and g.nbr[12].tolist() == [-1, 0, -1, -1]      # +x / -x
    assert g.nbr[0].tolist() == [2, -1, -1, -1] and g.nbr[26].tolist() == [-1, -1, 0, -1]       # the corners
    assert g.offsets_tensor().tolist() == [0, 5]


def test_grid_bookkeeping_many_scenes_and_empty_ones():
    a = centres([[0, 0, 0], [1, 0, 0]])
    b = centres([[0, 0, 0]])
    g = O.VoxelGrid.from_scenes([a, torch.zeros(0, 3, dtype=torch.float64), b], voxel_size=VS)
    assert g.offsets == [0, 2, 2, 3] and g.n_scenes == 3 and g.n_voxels == 3
    assert g.coords.tolist() == [[0, 0, 0, 0], [0, 1, 0, 0], [2, 0, 0, 0]]          # the same cell of two scenes: two voxels
    assert g.nbr[14].tolist() == [1, -1, -1]                                        # ... that are not neighbours
    g2 = O.VoxelGrid(torch.cat([a, b]), torch.tensor([0, 2, 2, 3]), voxel_size=VS)
    assert g2.offsets == g.offsets and torch.equal(g2.coords, g.coords)
    e = O.VoxelGrid(torch.zeros(0, 3), voxel_size=VS)
    assert e.n_points == 0 and e.n_voxels == 0 and e.nbr.shape == (27, 0)
    with pytest.raises(ValueError):
        O.VoxelGrid.from_scenes([])


def test_grid_argument_checks():
    xyz = centres([[0, 0, 0]])
    with pytest.raises(ValueError, match="connectivity"):
        O.VoxelGrid(xyz, connectivity=18)
    with pytest.raises(ValueError):
        O.VoxelGrid(xyz, voxel_size=0.0)
    with pytest.raises(TypeError):
        O.VoxelGrid(torch.zeros(3, 3, dtype=torch.int32))
    with pytest.raises(TypeError):
        O.VoxelGrid(torch.zeros(3, 2))
    with pytest.raises(ValueError, match="offsets"):
        O.VoxelGrid(xyz, [0, 2])
    with pytest.raises(ValueError, match="offsets"):
        O.VoxelGrid(centres([[0, 0, 0], [1, 1, 1]]), [0, 2, 1, 2])
    with pytest.raises(ValueError, match="32767"):
        O.VoxelGrid(torch.tensor([[0.0, 0.0, 32767 * VS]]), voxel_size=VS)
    with pytest.raises(ValueError, match="32767"):
        O.VoxelGrid(torch.tensor([[0.0, float("nan"), 0.0]]), voxel_size=VS)
    O.VoxelGrid(torch.tensor([[0.0, 0.0, 32766 * VS + 0.1], [-32766 * VS, 0.0, 0.0]]), voxel_size=VS)
    with pytest.raises(ValueError, match="2\\^22"):
        O.VoxelGrid(torch.zeros(1 << 22, 3), voxel_size=VS)


def test_find_objects_argument_checks():
    g = O.VoxelGrid(centres([[0, 0, 0], [1, 0, 0], [4, 4, 4]]), voxel_size=VS)
    heat = torch.ones(3, 2, dtype=torch.float16)
    with pytest.raises(TypeError):
        O.find_objects(g, heat.float(), 0.5)
    with pytest.raises(TypeError):
        O.find_objects(g, heat.numpy(), 0.5)
    with pytest.raises(TypeError):
        O.find_objects("grid", heat, 0.5)
    with pytest.raises(ValueError):
        O.find_objects(g, heat[:2], 0.5)
    with pytest.raises(ValueError):
        O.find_objects(g, heat[:, 0], 0.5)
    with pytest.raises(ValueError, match="device"):
        O.find_objects(g, heat.to("meta"), 0.5)
    with pytest.raises(ValueError, match="3 thresholds for 2"):
        O.find_objects(g, heat, [0.1, 0.2, 0.3])
    for m in (0, 65, -1):
        with pytest.raises(ValueError, match="max_objects"):
            O.find_objects(g, heat, 0.5, max_objects=m)
    with pytest.raises(ValueError, match="min_points"):
        O.find_objects(g, heat, 0.5, min_points=0)
    with pytest.raises(ValueError, match="names"):
        O.find_objects(g, heat, 0.5, names=["a", "b"])
    r = O.find_objects(g, heat, 0.5, max_objects=64)
    assert r.n_points.shape == (1, 2, 64) and r.point_object is None
    with pytest.raises(ValueError, match='by must be'):
        r.rank_scenes(0, by="volume")
    with pytest.raises(IndexError):
        r.rank_scenes(2)
    with pytest.raises(IndexError):
        r.objects(0, -1)


def test_objects_ordering_ties_padding_and_derived_fields():
    # scene "a": two objects with EQUAL peaks (ordered by the peak's row) and a weaker one; scene "b": nothing over the threshold
    a = centres([[0, 0, 0], [9, 9, 9], [9, 9, 9], [4, 0, 0], [0, 0, 1]])
    b = centres([[0, 0, 0], [1, 0, 0]])
    g = O.VoxelGrid.from_scenes([a, torch.zeros(0, 3, dtype=torch.float64), b], voxel_size=VS)
    heat = torch.tensor([[0.5], [0.75], [0.25], [0.125], [0.75], [0.0], [-1.0]], dtype=torch.float16)
    r = O.find_objects(g, heat, 0.125, max_objects=4, return_point_ids=True, names=["a", "empty", "b"])
    assert r.n_objects.tolist() == [[3], [0], [0]]
    objs = r.objects("a", 0)
    assert [o["peak_point"] for o in objs] == [1, 4, 3] and [o["peak_score"] for o in objs] == [0.75, 0.75, 0.125]
    assert [o["n_points"] for o in objs] == [2, 2, 1] and [o["n_voxels"] for o in objs] == [1, 2, 1]
    assert [o["rank"] for o in objs] == [0, 1, 2]
    assert objs[0]["mean_score"] == 0.5 and objs[1]["mean_score"] == 0.625
    assert objs[0]["centroid"] == [9.5 * VS] * 3 and objs[1]["centroid"] == [0.5 * VS, 0.5 * VS, 1.0 * VS]
    assert objs[1]["box_min"] == [0.25, 0.25, 0.25] and objs[1]["box_max"] == [0.25, 0.25, 0.75]
    assert r.objects("empty", 0) == [] and r.objects(2, 0) == []
    assert r.n_points[0, 0].tolist() == [2, 2, 1, 0] and r.peak_point[0, 0, 3].item() == -1
    assert r.peak_score[0, 0, 3].item() == float("-inf") and r.peak_point[1:].eq(-1).all() and r.n_points[1:].eq(0).all()
    assert r.point_object[:, 0].tolist() == [1, 0, 0, 2, 1, -1, -1]
    # the derived fields are the contract's formulas on the exact integers
    assert torch.equal(r.mean_score[0, 0, :3], r.score_sum[0, 0, :3].double() / 2 ** 24 / r.n_points[0, 0, :3].double())
    assert torch.equal(r.centroid[0, 0, :3], (r.vox_sum[0, 0, :3].double() / r.n_points[0, 0, :3, None].double() + 0.5) * VS)
    assert r.score_sum[0, 0].tolist() == [2 ** 24, int(1.25 * 2 ** 24), 2 ** 21, 0] and r.vox_sum[0, 0, 1].tolist() == [0, 0, 1]
    # min_points drops the single point; the cap keeps the best and still counts all that passed
    r2 = O.find_objects(g, heat, 0.125, min_points=2, max_objects=1, return_point_ids=True)
    assert r2.n_objects.tolist() == [[2], [0], [0]] and r2.peak_point[0, 0].tolist() == [1]
    assert r2.point_object[:, 0].tolist() == [-1, 0, 0, -1, -1, -1, -1]


def test_rank_scenes_orders_and_breaks_ties_in_scene_order():
    one = centres([[0, 0, 0]])
    two = centres([[0, 0, 0], [5, 5, 5], [5, 5, 6]])
    g = O.VoxelGrid.from_scenes([one, two, torch.zeros(0, 3, dtype=torch.float64), one], voxel_size=VS)
    heat = torch.tensor([[0.5, 0.0], [0.25, 0.0], [0.75, 0.0], [0.5, 0.0], [0.5, 0.0]], dtype=torch.float16)
    r = O.find_objects(g, heat, [0.25, 0.5], names=["one", "two", "none", "again"])
    assert r.rank_scenes(0) == [("two", 2), ("one", 1), ("again", 1), ("none", 0)]
    assert r.rank_scenes(0, by="peak") == [("two", 0.75), ("one", 0.5), ("again", 0.5), ("none", float("-inf"))]
    assert r.rank_scenes(0, by="largest") == [("two", 2), ("one", 1), ("again", 1), ("none", 0)]
    assert r.rank_scenes(1) == [("one", 0), ("two", 0), ("none", 0), ("again", 0)]
    assert r.rank_scenes(1, by="peak")[0] == ("one", float("-inf"))


def test_search_result_forwards_to_find_objects():
    gen = torch.Generator().manual_seed(3)
    bank = S.FeatureBank(8, CPU)
    fa = torch.nn.functional.normalize(torch.randn(6, 8, generator=gen), dim=1)
    fb = torch.nn.functional.normalize(torch.randn(4, 8, generator=gen), dim=1)
    bank.add_scene("a", fa)
    bank.add_scene("b", fb)
    xyz = torch.rand(10, 3, generator=gen, dtype=torch.float64) * 2
    g = O.VoxelGrid(xyz, bank.offsets, voxel_size=VS)
    t = torch.nn.functional.normalize(torch.randn(3, 8, generator=gen), dim=1).half()
    with pytest.raises(ValueError, match="return_heat"):
        S.search(bank, t).find_objects(g, 0.0)
    res = S.search(bank, t, return_heat=True)
    r = res.find_objects(g, 0.0, max_objects=3, return_point_ids=True)
    assert r.names == ["a", "b"] and r.n_points.shape == (2, 3, 3)
    direct = O.find_objects(g, res.heat, 0.0, max_objects=3, return_point_ids=True)
    for f in O.FIELDS + ("n_objects", "point_object"):
        assert torch.equal(getattr(r, f), getattr(direct, f))
    oref.assert_same(r, oref.find_objects(xyz, bank.offsets, res.heat, [0.0] * 3, voxel_size=VS, max_objects=3), VS)


def test_reference_connectivity_and_offsets():
    assert len(oref._offsets(26)) == 26 and len(oref._offsets(6)) == 6
    xyz = centres([[0, 0, 0], [1, 1, 0], [3, 0, 0], [4, 1, 1]])
    heat = torch.ones(4, 1, dtype=torch.float16)
    r26 = oref.find_objects(xyz, [0, 4], heat, [0.5], voxel_size=VS, connectivity=26)
    r6 = oref.find_objects(xyz, [0, 4], heat, [0.5], voxel_size=VS, connectivity=6)
    assert r26["n_objects"].item() == 2 and r6["n_objects"].item() == 4
    assert np.array_equal(r26["n_points"][0, 0, :3].numpy(), [2, 2, 0])
