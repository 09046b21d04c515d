"""Host logic of openscene_amd.neighbors WITHOUT a GPU: ops.knn_grid / ops.knn_blend / ops.knn_vote are replaced by the stand-ins
of tests/neighbors_reference.py (the kernels' contract in numpy) and the grid's ops by those of tests/objects_reference.py, so
PointIndex, knn, knn_self, Neighbors, transfer, fill_missing and smooth are the code under test; the wrappers' argument checks
run as they are (they come before the device check).  The reference's own invariants -- what tests/test_gpu_neighbors.py relies
on -- are checked here, on the same inputs."""
import os
import re

import numpy as np
import pytest
import torch

import neighbors_reference as nr
import objects_reference as oref
from openscene_amd import _lib
from openscene_amd import neighbors as N
from openscene_amd import ops
from openscene_amd.objects import VoxelGrid, find_objects

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = {"osn_knn_grid", "osn_knn_blend", "osn_knn_vote"}
REAL_GRID, REAL_BLEND, REAL_VOTE = ops.knn_grid, ops.knn_blend, ops.knn_vote


@pytest.fixture(autouse=True)
def cpu_kernels(monkeypatch):
    for name, f in (("coords_unique", oref.coords_unique), ("kmap_build", oref.kmap_build), ("objects_find", oref.objects_find),
                    ("knn_grid", nr.knn_grid), ("knn_blend", nr.knn_blend), ("knn_vote", nr.knn_vote)):
        monkeypatch.setattr(ops, name, f)


def grid_of(case):
    return VoxelGrid(torch.from_numpy(case["xyz"]), case["offsets"], voxel_size=case["voxel_size"])


def same(got, ref):
    idx, dist, count = ref
    assert np.array_equal(got.count.numpy(), count)
    assert np.array_equal(got.idx.numpy(), idx)
    assert np.array_equal(got.dist2.numpy().view(np.uint32), dist.view(np.uint32))


# ---------------------------------------------------------------------------------------------------- the header
def test_the_header_declares_exactly_the_new_entries_the_prototypes_list():
    src = open(os.path.join(ROOT, "include", "openscene_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = {n for n in re.findall(r"\b(osn_[a-z0-9_]+)\s*\(", code) if n.startswith("osn_knn_")}
    assert declared == NEW_ENTRIES == {n for n in _lib.PROTOTYPES if n.startswith("osn_knn_")}
    for name in NEW_ENTRIES:                                                 # the argument counts agree
        decl = re.search(name + r"\s*\((.*?)\);", code, flags=re.S).group(1)
        assert len(decl.split(",")) == len(_lib.PROTOTYPES[name][1]), name
    block = src[src.index("csrc/neighbors.hip"):src.index("int osn_knn_grid(")]
    for word in ("run/evaluate.py:297-300", "bits(d2) << 32 | point index", "d2 <= r2", "-1 past count", "+inf past count", "smallest j"):
        assert word in block, word
    assert "neighbors.hip" in open(os.path.join(ROOT, "openscene_amd", "build.py")).read()


# ---------------------------------------------------------------------------------------------------- the reference itself
def test_the_27_cells_lose_nothing_against_all_pairs_on_the_random_case():
    c = nr.random_case()
    ref = nr.knn(c["xyz"], c["offsets"], c["voxel_size"], c["queries"], c["qscene"], c["k"], c["radius"])
    brute = nr.knn_brute(c["xyz"], c["offsets"], c["queries"], c["qscene"], c["k"], c["radius"])
    for a, b in zip(ref, brute):
        assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
    count = ref[2]
    # what the seed was chosen for: full lists, short lists, and at least half of the queries with a neighbour
    assert nr.RANDOM_SEED == 5
    assert (count == c["k"]).sum() >= 20 and ((count > 0) & (count < c["k"])).sum() >= 20 and (count == 0).sum() >= 1
    assert (count >= 1).sum() * 2 >= count.shape[0]
    for s in (0, 1):                                                         # never a neighbour of the other scene
        got = ref[0][c["qscene"] == s]
        got = got[got >= 0]
        assert (got >= c["offsets"][s]).all() and (got < c["offsets"][s + 1]).all()


@pytest.mark.parametrize("dtype", [np.float16, np.float32])
@pytest.mark.parametrize("weights", ["uniform", "inverse"])
def test_the_reference_blend_stays_within_the_bound_against_float64(dtype, weights):
    c = nr.random_case()
    idx, dist, count = nr.knn(c["xyz"], c["offsets"], c["voxel_size"], c["queries"][:300], c["qscene"][:300], c["k"], c["radius"])
    values = c["values"].astype(dtype)
    out, found = nr.blend(values, idx, dist, count, weights, c["voxel_size"], fill=7)
    exact, absum = nr.blend_exact(values, idx, dist, count, weights, c["voxel_size"])
    bound = nr.blend_bound(exact, absum, count, dtype)
    assert np.array_equal(found, count > 0) and (out[~found] == 7).all()
    err = np.abs(out.astype(np.float64) - exact)[found]
    assert (err <= bound[found]).all(), float((err / bound[found]).max())
    assert err.max() > 0                                                     # (the check is not vacuous)


def test_the_reference_vote_on_hand_made_lists():
    labels = np.array([3, 3, 5, 5, -1, 7, -2], dtype=np.int64)
    idx = np.array([[2, 0, 1, 3], [2, 0, 1, 4], [4, 6, -1, -1], [4, 5, 6, -1], [0, 2, -1, -1], [5, -1, -1, -1]], dtype=np.int32)
    count = np.array([4, 4, 2, 3, 2, 0], dtype=np.int32)
    # a 2 : 2 tie goes to the nearer first holder; 2 : 1; only ignored labels; one label among ignored ones; 1 : 1; nothing
    assert nr.vote(labels, idx, count, fill=-9).tolist() == [5, 3, -9, 7, 3, -9]


# ---------------------------------------------------------------------------------------------------- the cases
def test_the_cases_hold_what_the_gpu_tests_rely_on():
    c = nr.lattice_case()
    idx, dist, count = nr.knn(c["xyz"], c["offsets"], 1.0, c["queries"], c["qscene"], 16, 1.0)
    assert (count == 16).any() and ((count > 0) & (count < 16)).any()
    valid = idx >= 0
    assert (dist[valid] == np.float32(1.0)).any()                            # points at exactly d2 == r2 are kept
    ties = (dist[:, 1:] == dist[:, :-1]) & valid[:, 1:]
    assert ties.sum() >= 50 and (idx[:, 1:][ties] > idx[:, :-1][ties]).all()  # equal d2: ascending point index
    assert (c["queries"][40:70] == np.floor(c["queries"][40:70])).all() and (c["queries"] < 0).any()      # cell faces, negative coordinates
    assert len({tuple(p) for p in c["xyz"]}) <= c["xyz"].shape[0] - 20       # duplicates
    for k in (1, 2, 4):                                                      # the exact means are taken where count is 1, 2 or 4
        cnt = nr.knn(c["xyz"], c["offsets"], 1.0, c["queries"], c["qscene"], k, 1.0)[2]
        assert (cnt == k).sum() >= 50
    votes = nr.vote(c["labels"], idx[:, :4], np.minimum(count, 4))
    assert (votes == -1).any() and (votes >= 0).any()
    c = nr.crowded_case()
    idx, dist, count = nr.knn(c["xyz"], c["offsets"], c["voxel_size"], c["queries"], c["qscene"], 16, c["radius"])
    assert count.tolist()[0] == 16 and count.tolist()[3] == 2 and sorted(idx[3].tolist()[:2]) == [300, 301] and np.isinf(dist[3, 2:]).all()
    c = nr.empty_case()
    count = nr.knn(c["xyz"], c["offsets"], c["voxel_size"], c["queries"], c["qscene"], 4, c["radius"])[2]
    assert count[:-1].tolist() == [0] * 8 and count[-1] > 0
    c = nr.room_case()
    assert 0.05 < (~c["seen"]).mean() < 0.2 and (c["heat"][~c["seen"]] > 0.5).sum() > 20


# ---------------------------------------------------------------------------------------------------- the CSR
def test_the_csr_lists_ascending_points_per_cell_and_respects_the_mask():
    c = nr.random_case()
    grid = grid_of(c)
    rng = np.random.default_rng(0)
    mask = rng.random(3000) < 0.4
    for sources in (None, mask):
        index = N.PointIndex(grid, None if sources is None else torch.from_numpy(sources))
        start, pts, inv = index.cell_start.numpy(), index.cell_points.numpy(), grid.inverse.numpy()
        assert index.cell_start.dtype == torch.int32 and index.cell_points.dtype == torch.int32
        assert start[0] == 0 and start[-1] == pts.shape[0] == (3000 if sources is None else mask.sum()) and start.shape[0] == grid.n_voxels + 1
        for v in range(grid.n_voxels):
            seg = pts[start[v]:start[v + 1]]
            want = np.nonzero((inv == v) & (True if sources is None else mask))[0]
            assert np.array_equal(seg, want)                                 # (np.nonzero ascends)
        assert index.table is grid.table and grid.table is not None
    empty = VoxelGrid(torch.zeros((0, 3)), None, voxel_size=0.1)
    index = N.PointIndex(empty)
    assert index.cell_start.tolist() == [0] and index.cell_points.shape[0] == 0 and empty.table is None
    res = index.knn(torch.zeros((3, 3)), 2)
    assert res.count.tolist() == [0, 0, 0] and (res.idx == -1).all() and torch.isinf(res.dist2).all()


# ---------------------------------------------------------------------------------------------------- host logic
@pytest.mark.parametrize("name", ["lattice", "crowded", "two_scene", "empty"])
def test_knn_of_foreign_queries_is_the_reference(name):
    c = getattr(nr, name + "_case")()
    index = N.PointIndex(grid_of(c))
    for k in (1, 5):
        got = index.knn(torch.from_numpy(c["queries"]), k, radius=c["radius"], scene=torch.from_numpy(c["qscene"]))
        same(got, nr.knn(c["xyz"], c["offsets"], c["voxel_size"], c["queries"], c["qscene"], k, c["radius"]))


def test_knn_self_exclude_and_sources():
    c = nr.lattice_case()
    grid = grid_of(c)
    n = c["xyz"].shape[0]
    mask = np.random.default_rng(1).random(n) < 0.5
    scene = np.zeros(n, dtype=np.int64)
    own = np.arange(n, dtype=np.int32)
    for sources in (None, mask):
        index = N.PointIndex(grid, None if sources is None else torch.from_numpy(sources))
        same(index.knn_self(4), nr.knn(c["xyz"], c["offsets"], 1.0, c["xyz"], scene, 4, 1.0, sources=sources))
        same(index.knn_self(4, include_self=False), nr.knn(c["xyz"], c["offsets"], 1.0, c["xyz"], scene, 4, 1.0, sources=sources, exclude=own))
        ex = torch.from_numpy(np.random.default_rng(2).integers(0, n, 100).astype(np.int32))
        same(index.knn(torch.from_numpy(c["queries"]), 4, exclude=ex),
             nr.knn(c["xyz"], c["offsets"], 1.0, c["queries"], c["qscene"], 4, 1.0, sources=sources, exclude=ex.numpy()))


def test_fill_missing_transfer_and_smooth_on_the_room():
    c = nr.room_case()
    grid = grid_of(c)
    heat, holed, seen = torch.from_numpy(c["heat"]), torch.from_numpy(c["holed"]), torch.from_numpy(c["seen"])
    filled, missing = N.fill_missing(grid, holed, seen, k=4)
    unseen = ~c["seen"]
    idx, dist, count = nr.knn(c["xyz"], c["offsets"], 0.05, c["xyz"][unseen], 0, 4, sources=c["seen"])
    ref, found = nr.blend(c["holed"], idx, dist, count, "inverse", 0.05)
    assert torch.equal(filled[seen].view(torch.int16), holed[seen].view(torch.int16))
    assert np.array_equal(filled.numpy()[unseen].view(np.uint16), ref.view(np.uint16))
    assert np.array_equal(missing.numpy()[unseen], ~found) and not missing.numpy()[c["seen"]].any() and (filled[missing] == 0).all()
    assert int(find_objects(grid, holed, c["threshold"]).n_objects[0, 0]) >= 2
    assert int(find_objects(grid, filled, c["threshold"]).n_objects[0, 0]) == 1
    out, found = N.transfer(N.PointIndex(grid), torch.from_numpy(c["xyz"]), heat, k=1)
    assert found.all() and torch.equal(out.view(torch.int16), heat.view(torch.int16))
    sm = N.smooth(grid, heat.float(), k=8)
    assert sm.shape == heat.shape and float(sm.min()) >= float(heat.min()) - 1e-6 and float(sm.max()) <= float(heat.max()) + 1e-6
    assert len({float(x) for x in sm.flatten()}) > 2                         # the object's rim is blended


# ---------------------------------------------------------------------------------------------------- argument checks
def test_the_surface_refuses_bad_arguments():
    c = nr.two_scene_case()
    grid = grid_of(c)
    index = N.PointIndex(grid)
    q = torch.from_numpy(c["queries"])
    for k in (0, 17):
        with pytest.raises(ValueError):
            index.knn(q, k)
        with pytest.raises(ValueError):
            index.knn_self(k)
    for radius in (0.0, -1.0, 0.1001, float("nan")):
        with pytest.raises(ValueError):
            index.knn(q, 1, radius=radius)
    with pytest.raises(TypeError):
        index.knn(q.long(), 1)
    with pytest.raises(ValueError):
        index.knn(q[:, :2], 1)
    with pytest.raises(ValueError):
        index.knn(q, 1, scene=torch.zeros(5, dtype=torch.int64))            # a scene vector of the wrong length
    with pytest.raises(TypeError):
        index.knn(q, 1, scene=torch.zeros(q.shape[0], dtype=torch.int32))
    with pytest.raises(TypeError):
        index.knn(q, 1, exclude=torch.zeros(q.shape[0], dtype=torch.int64))
    with pytest.raises(TypeError):
        N.PointIndex(grid, torch.zeros(300, dtype=torch.uint8))
    with pytest.raises(ValueError):
        N.PointIndex(grid, torch.zeros(299, dtype=torch.bool))
    with pytest.raises(TypeError):
        N.PointIndex("grid")
    nb = index.knn(q, 2)
    with pytest.raises(ValueError):
        nb.blend(torch.zeros((300, 4)), weights="gaussian")
    with pytest.raises(TypeError):
        nb.blend(torch.zeros((300, 4), dtype=torch.float64))
    with pytest.raises(ValueError):
        nb.blend(torch.zeros((299, 4)))
    with pytest.raises(ValueError):
        nb.blend(torch.zeros(300))
    with pytest.raises(TypeError):
        nb.vote(torch.zeros(300, dtype=torch.int32))
    with pytest.raises(ValueError):
        nb.vote(torch.zeros(299, dtype=torch.int64))
    with pytest.raises(TypeError):
        N.fill_missing(grid, torch.zeros((300, 4)), torch.zeros(300))
    with pytest.raises(TypeError):
        N.transfer(grid, q, torch.zeros((300, 4)))


def test_an_fp8_bank_is_refused():
    from openscene_amd.search import FeatureBank
    c = nr.two_scene_case()
    grid = grid_of(c)
    bank = FeatureBank(16, torch.device("cpu"), capacity_rows=300, dtype="fp8")
    with pytest.raises(TypeError):
        N.fill_missing(grid, bank, torch.ones(300, dtype=torch.bool))


def test_the_wrappers_refuse_bad_arguments():
    xyz = torch.zeros((5, 3))
    start, pts = torch.zeros(3, dtype=torch.int32), torch.zeros(5, dtype=torch.int32)
    nbr = torch.full((27, 2), -1, dtype=torch.int32)
    q, col = torch.zeros((4, 3)), torch.zeros(4, dtype=torch.int32)
    ok = dict(xyz=xyz, cell_start=start, cell_points=pts, nbr=nbr, query_xyz=q, q_cell=col, k=4, r2=0.01)
    for bad, exc in ((dict(xyz=xyz.double()), TypeError), (dict(xyz=xyz[:, :2].contiguous()), ValueError), (dict(cell_start=start.long()), TypeError),
                     (dict(cell_points=torch.zeros(6, dtype=torch.int32)), ValueError), (dict(nbr=nbr.long()), TypeError),
                     (dict(nbr=nbr[:26].contiguous()), ValueError), (dict(nbr=torch.full((2, 27), -1, dtype=torch.int32).t()), ValueError),
                     (dict(query_xyz=q.half()), TypeError), (dict(query_xyz=q[:, :2].contiguous()), ValueError), (dict(q_cell=col.long()), TypeError),
                     (dict(q_cell=col[:3]), ValueError), (dict(k=0), ValueError), (dict(k=17), ValueError), (dict(r2=-1.0), ValueError),
                     (dict(r2=float("nan")), ValueError), (dict(r2=float("inf")), ValueError), (dict(exclude=col.long()), TypeError),
                     (dict(order=col[:2]), ValueError), (dict(err=torch.zeros(2, dtype=torch.int32)), ValueError)):
        with pytest.raises(exc):
            REAL_GRID(**dict(ok, **bad))
    with pytest.raises(_lib.OpenSceneAmdError):                              # every check passed: only the device is missing
        REAL_GRID(**ok)
    values = torch.zeros((5, 3), dtype=torch.float16)
    idx, d2, cnt = torch.zeros((4, 2), dtype=torch.int32), torch.zeros((4, 2)), torch.zeros(4, dtype=torch.int32)
    for args, exc in (((values.double(), idx, d2, cnt), TypeError), ((values[:, 0], idx, d2, cnt), ValueError), ((values, idx.long(), d2, cnt), TypeError),
                      ((values, idx, d2.half(), cnt), TypeError), ((values, idx, d2[:3], cnt), ValueError), ((values, idx, d2, cnt[:3]), ValueError),
                      ((values, torch.zeros((4, 17), dtype=torch.int32), torch.zeros((4, 17)), cnt), ValueError)):
        with pytest.raises(exc):
            REAL_BLEND(*args)
    with pytest.raises(ValueError):
        REAL_BLEND(values, idx, d2, cnt, inverse=True, eps=0.0)
    with pytest.raises(_lib.OpenSceneAmdError):
        REAL_BLEND(values, idx, d2, cnt)
    labels = torch.zeros(5, dtype=torch.int64)
    for args, exc in (((labels.int(), idx, cnt), TypeError), ((labels[:, None], idx, cnt), ValueError), ((labels, idx.long(), cnt), TypeError),
                      ((labels, idx, cnt.long()), TypeError), ((labels, idx, cnt[:3]), ValueError)):
        with pytest.raises(exc):
            REAL_VOTE(*args)
    with pytest.raises(_lib.OpenSceneAmdError):
        REAL_VOTE(labels, idx, cnt)
