"""Host logic of the GPU Point3DLoader (openscene_amd.loader.PointLoader / point_item / point_collate,
TrainAugmentation.prevoxel_apply, ops.elastic_distort) WITHOUT a GPU: tests/cpu_backend.py stands in for the voxeliser and
batch ops, and the three elastic-distortion kernels are replaced by a scipy restatement (the calls
dataset/augmentation.py:181-194 makes).  Checked against the reference's real Point3DLoader
(tests/golden/loader_point.npz): the random draws happen in the same order, with the same sizes."""
import numpy as np
import pytest
import torch

import cpu_backend
import point_loader_cases as plc


def _bbox(xyz):
    x = xyz.numpy()
    return torch.from_numpy(np.concatenate([x.min(0), x.max(0)]))


def _blur(noise):
    from scipy import ndimage
    g = noise.numpy()
    bx = np.ones((3, 1, 1, 1)).astype("float32") / 3
    by = np.ones((1, 3, 1, 1)).astype("float32") / 3
    bz = np.ones((1, 1, 3, 1)).astype("float32") / 3
    for _ in range(2):
        g = ndimage.convolve(g, bx, mode="constant", cval=0)
        g = ndimage.convolve(g, by, mode="constant", cval=0)
        g = ndimage.convolve(g, bz, mode="constant", cval=0)
    noise.copy_(torch.from_numpy(g))
    return noise


def _apply(xyz, noise, axes, magnitude):
    from scipy.interpolate import RegularGridInterpolator
    x = xyz.numpy()
    out = x + RegularGridInterpolator([np.asarray(a) for a in axes], noise.numpy(), bounds_error=0, fill_value=0)(x) * magnitude
    return torch.from_numpy(out), _bbox(torch.from_numpy(out))


@pytest.fixture
def cpu_ops(monkeypatch):
    from openscene_amd import ops
    cpu_backend.install(monkeypatch)
    calls = []

    def apply(*a):
        calls.append(a[1].shape)
        return _apply(*a)
    monkeypatch.setattr(ops, "bbox", _bbox)
    monkeypatch.setattr(ops, "elastic_blur", _blur)
    monkeypatch.setattr(ops, "elastic_apply", apply)
    return calls


@pytest.mark.parametrize("case", plc.CASES, ids=[c[0] for c in plc.CASES])
def test_point_loader_matches_the_reference_point_loader(cpu_ops, golden_dir, tmp_path, case):
    d = plc.load(golden_dir)
    plc.write_scenes(d, tmp_path)
    plc.check(d, plc.run(d, tmp_path, torch.device("cpu"), case), case)
    assert (len(cpu_ops) > 0) == case[3]                   # the distortion ran exactly in the augmented cases


def test_elastic_distort_host_steps(cpu_ops, golden_dir):
    """ops.elastic_distort's host part (grid size from the box, the numpy draw, np.linspace axes) and prevoxel_apply's
    gate and chaining reproduce ElasticDistortion with the same seeds -- points on grid nodes and on the last node."""
    import random
    from openscene_amd import ops
    from openscene_amd.loader import TrainAugmentation
    d = plc.load(golden_dir)
    x = torch.from_numpy(d["elastic_x"])
    np.random.seed(51)
    assert np.array_equal(ops.elastic_distort(x, 0.2, 0.4).numpy(), d["elastic_one"])
    assert tuple(cpu_ops[-1][:3]) == (22, 17, 15)            # LAST_NODE_K + 2 nodes: the last one is the cloud's maximum
    np.random.seed(53)
    random.seed(53)
    out = TrainAugmentation().prevoxel_apply(x)
    assert np.array_equal(out.numpy(), d["elastic_two"])
    np.random.seed(51)
    out, box = ops.elastic_distort(x, 0.2, 0.4, return_bbox=True)
    assert np.array_equal(box.numpy(), np.concatenate([d["elastic_one"].min(0), d["elastic_one"].max(0)]))


def test_prevoxel_apply_gate_and_none():
    import random
    from openscene_amd.loader import TrainAugmentation
    x = torch.zeros(4, 3, dtype=torch.float64)
    assert TrainAugmentation(elastic_params=None).prevoxel_apply(x) is x
    for s in range(200):
        random.seed(s)
        if random.random() >= 0.95:
            break
    random.seed(s)
    state = np.random.get_state()[1].copy()
    assert TrainAugmentation().prevoxel_apply(x) is x       # gate closed: no numpy draw, no kernel
    assert np.array_equal(np.random.get_state()[1], state)


def test_point_loader_length_loop_and_wrap(cpu_ops, golden_dir, tmp_path):
    from openscene_amd.loader import PointLoader
    d = plc.load(golden_dir)
    plc.write_scenes(d, tmp_path)
    root = str(tmp_path / "room")
    ds = PointLoader(root, voxel_size=0.05, split="val", loop=3, memcache_init=True, identifier=7, device="cpu")
    assert len(ds) == 6 and len(ds.data_paths) == 2
    assert ds.SCALE_AUGMENTATION_BOUND == (0.9, 1.1) and ds.ELASTIC_DISTORT_PARAMS == ((0.2, 0.4), (0.8, 1.6))
    for i in (0, 1):
        np.random.seed(3)
        a = ds[i]
        np.random.seed(3)
        b = ds[i + 4]                                        # index % len(data_paths)
        assert all(torch.equal(u, v) for u, v in zip(a, b))
        assert a[0].shape[0] == np.unique(a[0].numpy(), axis=0).shape[0]
    with pytest.raises(Exception, match="0 file"):
        PointLoader(str(tmp_path / "nothing"), split="train", device="cpu")


def test_point_collate_offsets(cpu_ops):
    from openscene_amd.loader import point_collate
    g = torch.Generator().manual_seed(0)
    items3, items4 = [], []
    for n_vox, n_pts in ((5, 9), (3, 4), (7, 7)):
        c = torch.randint(0, 50, (n_vox, 3), generator=g, dtype=torch.int32)
        f = torch.randn(n_vox, 3, generator=g)
        items3.append((c, f, torch.arange(n_vox)))
        items4.append((c, f, torch.arange(n_pts), torch.randint(0, n_vox, (n_pts,), generator=g)))
    coords, feats, labels = point_collate(items3)
    assert coords.dtype == torch.int32 and coords.shape == (15, 4)
    assert coords[:, 0].tolist() == [0] * 5 + [1] * 3 + [2] * 7
    assert torch.equal(coords[:, 1:], torch.cat([it[0] for it in items3])) and feats.shape == (15, 3)
    assert torch.equal(labels, torch.cat([it[2] for it in items3]))
    coords, feats, labels, rec = point_collate(items4)
    assert labels.shape == (20,)
    assert torch.equal(rec, torch.cat([items4[0][3], items4[1][3] + 5, items4[2][3] + 8]))
    with pytest.raises(ValueError):
        point_collate([])
    with pytest.raises(ValueError):
        point_collate([items3[0], items4[1]])


def test_load_scene_missing_colour(tmp_path):
    from openscene_amd import io
    xyz = np.random.default_rng(0).random((10, 3))
    io.save_scene(tmp_path / "l.pth", xyz, 0, np.zeros(10))
    assert np.array_equal(io.load_scene(tmp_path / "l.pth")[1], np.zeros((10, 3)))
    c = io.load_scene(tmp_path / "l.pth", missing_color=127.5)[1]
    assert c.dtype == np.float64 and np.array_equal(c, np.full((10, 3), 127.5))
