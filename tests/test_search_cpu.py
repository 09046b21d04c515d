"""Host logic of openscene_amd.search WITHOUT a GPU: the two kernels (ops.bank_append, ops.bank_search) are replaced by
the torch stand-ins of tests/search_reference.py; everything else -- the bank's bookkeeping, the files, the argument
checks, SearchResult.rank_scenes -- is the code under test."""
import os

import numpy as np
import pytest
import torch

import search_reference as sr
from openscene_amd import io as osn_io
from openscene_amd import ops
from openscene_amd import search as S

CPU = torch.device("cpu")


@pytest.fixture(autouse=True)
def cpu_kernels(monkeypatch):
    monkeypatch.setattr(ops, "bank_append", sr.bank_append)
    monkeypatch.setattr(ops, "bank_check", sr.bank_check)
    monkeypatch.setattr(ops, "bank_search", sr.bank_search)


def unit(n, d, gen):
    return torch.nn.functional.normalize(torch.randn(n, d, generator=gen), dim=1)


def test_bank_bookkeeping_growth_empty_scene_and_duplicate_name():
    g = torch.Generator().manual_seed(0)
    bank = S.FeatureBank(16, CPU, capacity_rows=8)
    a = unit(5, 16, g)
    b = unit(40, 16, g).half()
    inv = torch.tensor([4, 0, 0, 3, 2, 1, 4])
    assert bank.add_scene("a", a, inv) == 0
    assert bank.add_scene("empty", torch.zeros(0, 16, dtype=torch.float16)) == 1
    assert bank.add_scene("b", b) == 2                       # past the capacity: the bank grows, earlier rows survive
    assert bank.offsets == [0, 7, 7, 47] and bank.names == ["a", "empty", "b"] and len(bank) == 3
    assert bank.rows == 47 and bank.capacity_rows >= 47 and bank.scene_rows() == [7, 0, 40]
    assert sr.same_bits(bank.scene("a"), a[inv].half()) and sr.same_bits(bank.scene(2), b)
    assert bank.scene("empty").shape == (0, 16)
    assert bank.offsets_tensor().tolist() == [0, 7, 7, 47]
    with pytest.raises(ValueError, match="already holds"):
        bank.add_scene("a", a)
    assert bank.offsets == [0, 7, 7, 47]


def test_bad_index_raises_and_leaves_the_bank_as_it_was():
    g = torch.Generator().manual_seed(1)
    bank = S.FeatureBank(8, CPU, capacity_rows=64)
    bank.add_scene("a", unit(6, 8, g))
    before = bank.features.clone()
    for bad in (-1, 6):
        with pytest.raises(RuntimeError):
            bank.add_scene("b", unit(6, 8, g), torch.tensor([0, bad, 2]))
        assert bank.offsets == [0, 6] and bank.names == ["a"] and sr.same_bits(bank.features, before)
    bank.add_scene("b", unit(6, 8, g), torch.tensor([0, 5, 2]))          # the error word was cleared
    assert bank.offsets == [0, 6, 9]


def test_argument_errors():
    g = torch.Generator().manual_seed(2)
    with pytest.raises(ValueError):
        S.FeatureBank(12, CPU)
    bank = S.FeatureBank(16, CPU)
    with pytest.raises(ValueError):
        bank.add_scene("x", unit(4, 8, g))
    with pytest.raises(TypeError):
        bank.add_scene("x", unit(4, 16, g).double())
    with pytest.raises(TypeError):
        bank.add_scene("x", unit(4, 16, g), torch.tensor([0.0, 1.0]))
    bank.add_scene("x", unit(4, 16, g))
    t = unit(3, 16, g).half()
    with pytest.raises(TypeError):
        S.search(bank, t.float())
    with pytest.raises(TypeError):
        S.search(bank, t.numpy())
    with pytest.raises(ValueError):
        S.search(bank, t[:, :8])
    with pytest.raises(ValueError):
        S.search(bank, t[0])
    with pytest.raises(ValueError):
        S.search(bank, t, k=0)
    with pytest.raises(ValueError):
        S.search(bank, t, k=129)
    with pytest.raises(ValueError):
        S.search(bank, t, thresholds=[0.1, 0.2])
    with pytest.raises(TypeError):
        S.search(bank.features, t)
    res = S.search(bank, t, thresholds=0.1)
    with pytest.raises(ValueError):
        res.rank_scenes(0, by="median")
    with pytest.raises(IndexError):
        res.rank_scenes(3)
    with pytest.raises(ValueError):
        S.search(bank, t).rank_scenes(0, by="count")
    with pytest.raises(ValueError):
        S.search(bank, t).scene_heat(0)


def test_save_load_round_trip(tmp_path):
    g = torch.Generator().manual_seed(3)
    bank = S.FeatureBank(16, CPU, capacity_rows=4)
    bank.add_scene("s0", unit(9, 16, g))
    bank.add_scene("s1", torch.zeros(0, 16))
    bank.add_scene("s2", (unit(30, 16, g) * 3).half())
    path = str(tmp_path / "bank.pt")
    bank.save(path)
    back = S.FeatureBank.load(path, CPU)
    assert back.dim == 16 and back.offsets == bank.offsets and back.names == bank.names
    assert sr.same_bits(back.features, bank.features)
    back.add_scene("s3", unit(2, 16, g))                      # still a working bank
    assert back.offsets == [0, 9, 9, 39, 41]


@pytest.mark.parametrize("dtype", [np.float32, np.float16])
def test_saved_point_features_come_back_with_name_and_values(tmp_path, dtype):
    g = torch.Generator().manual_seed(4)
    folder = str(tmp_path / "feats")
    scenes = {"scene0011_00_vh_clean_2": unit(12, 16, g), "scene0015_00_vh_clean_2": unit(7, 16, g) * 2}
    for name, f in scenes.items():
        p = osn_io.save_point_features(folder, name, "ensemble", f.numpy().astype(dtype))
        assert os.path.basename(p) == name + "_openscene_feat_ensemble.npy"
        back = np.load(p)
        assert back.dtype == dtype and back.shape == tuple(f.shape)            # np.save layout, dtype kept
    osn_io.save_point_features(folder, "scene0011_00_vh_clean_2", "distill", scenes["scene0011_00_vh_clean_2"])   # another type: not read
    bank = S.FeatureBank(16, CPU)
    assert bank.add_saved(folder, "ensemble") == sorted(scenes)
    assert bank.names == sorted(scenes) and bank.offsets == [0, 12, 19]
    for name, f in scenes.items():
        assert sr.same_bits(bank.scene(name), torch.from_numpy(f.numpy().astype(dtype)).half())
    assert [n for n, _ in osn_io.list_point_features(folder, "distill")] == ["scene0011_00_vh_clean_2"]


def test_search_result_shapes_padding_and_heat():
    g = torch.Generator().manual_seed(5)
    bank = S.FeatureBank(16, CPU)
    bank.add_scene("short", unit(3, 16, g))
    bank.add_scene("none", torch.zeros(0, 16))
    bank.add_scene("long", unit(50, 16, g))
    t = unit(2, 16, g).half()
    res = S.search(bank, t, k=8, thresholds=[0.0, 0.2], return_heat=True)
    assert res.topk_scores.shape == (3, 2, 8) and res.topk_points.shape == (3, 2, 8) and res.counts.shape == (3, 2)
    assert res.heat.shape == (53, 2) and res.scene_heat("long").shape == (50, 2)
    assert (res.topk_points[0, :, 3:] == -1).all() and torch.isinf(res.topk_scores[0, :, 3:].float()).all()
    assert (res.topk_points[0, :, :3] >= 0).all()
    assert (res.topk_points[1] == -1).all() and (res.topk_scores[1].float() == float("-inf")).all()
    assert (res.topk_points[2] >= 0).all() and res.counts[1].tolist() == [0, 0]
    assert S.search(bank, t, k=8).heat is None and S.search(bank, t, k=8).counts is None
    hm = S.heat_map(unit(5, 16, g), t, torch.tensor([1, 1, 4, 0]))
    assert hm.shape == (4, 2) and hm.dtype == torch.float16 and sr.same_bits(hm[0], hm[1])


def test_rank_scenes_each_criterion_with_ties():
    names = ["a", "b", "c", "d"]
    inf = float("-inf")
    top_s = torch.tensor([[[0.5, 0.25]], [[0.75, 0.0]], [[0.5, 0.5]], [[inf, inf]]], dtype=torch.float16)
    top_p = torch.tensor([[[3, 1]], [[0, 2]], [[7, -1]], [[-1, -1]]])
    counts = torch.tensor([[4], [9], [9], [0]])
    res = S.SearchResult(names, [0, 10, 20, 30, 30], top_s, top_p, counts, None)
    assert res.rank_scenes(0, by="max") == [("b", 0.75), ("a", 0.5), ("c", 0.5), ("d", inf)]          # a before c: scene order
    assert res.rank_scenes(0, by="topk_mean") == [("c", 0.5), ("a", 0.375), ("b", 0.375), ("d", inf)]   # c: one valid score
    assert res.rank_scenes(0, by="count") == [("b", 9), ("c", 9), ("a", 4), ("d", 0)]
    assert res.rank_scenes(0) == res.rank_scenes(0, by="max")
