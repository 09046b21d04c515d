"""HIP elastic distortion (csrc/elastic.hip) and the GPU Point3DLoader (openscene_amd.loader.PointLoader) -- bit for bit
against numpy / scipy and against the reference's real Point3DLoader (tests/golden/loader_point.npz)."""
import random

import numpy as np
import pytest
import torch
from scipy import ndimage
from scipy.interpolate import RegularGridInterpolator

import point_loader_cases as plc

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda", 0)


def ref_blur(noise):
    bx = np.ones((3, 1, 1, 1)).astype("float32") / 3
    by = np.ones((1, 3, 1, 1)).astype("float32") / 3
    bz = np.ones((1, 1, 3, 1)).astype("float32") / 3
    for _ in range(2):
        noise = ndimage.convolve(noise, bx, mode="constant", cval=0)
        noise = ndimage.convolve(noise, by, mode="constant", cval=0)
        noise = ndimage.convolve(noise, bz, mode="constant", cval=0)
    return noise


def ref_field(coords, granularity, magnitude):
    """ElasticDistortion.elastic_distortion (dataset/augmentation.py:159-194), the same numpy / scipy calls."""
    coords_min = coords.min(0)
    noise_dim = ((coords - coords_min).max(0) // granularity).astype(int) + 3
    noise = ref_blur(np.random.randn(*noise_dim, 3).astype(np.float32))
    ax = [np.linspace(d_min, d_max, d) for d_min, d_max, d in
          zip(coords_min - granularity, coords_min + granularity * (noise_dim - 2), noise_dim)]
    interp = RegularGridInterpolator(ax, noise, bounds_error=0, fill_value=0)
    return coords + interp(coords) * magnitude


def room(n=550000, seed=5):
    """A ScanNet-sized room over 8 x 6 x 3 m: a quarter of the points on the floor, a quarter on two walls."""
    rng = np.random.default_rng(seed)
    x = rng.random((n, 3)) * np.asarray((8.0, 6.0, 3.0)) - np.asarray((1.0, 2.0, 0.0))
    x[: n // 4, 2] = rng.normal(0, 0.01, n // 4)
    x[n // 4: 2 * (n // 4), 0] = np.where(rng.random(n // 4) < 0.5, -1.0, 7.0) + rng.normal(0, 0.01, n // 4)
    return x


@pytest.mark.parametrize("case", plc.CASES, ids=[c[0] for c in plc.CASES])
def test_point_loader_matches_the_reference_point_loader(golden_dir, tmp_path, case):
    d = plc.load(golden_dir)
    plc.write_scenes(d, tmp_path)
    plc.check(d, plc.run(d, tmp_path, dev(), case), case)


def test_elastic_fixture_grid_nodes_and_last_node(golden_dir):
    from openscene_amd import ops
    from openscene_amd.loader import TrainAugmentation
    d = plc.load(golden_dir)
    x = torch.from_numpy(d["elastic_x"]).to(dev())
    np.random.seed(51)
    assert np.array_equal(ops.elastic_distort(x, 0.2, 0.4).cpu().numpy(), d["elastic_one"])
    np.random.seed(53)
    random.seed(53)
    assert np.array_equal(TrainAugmentation().prevoxel_apply(x).cpu().numpy(), d["elastic_two"])


@pytest.mark.parametrize("shape", [(3, 3, 3), (5, 7, 9), (1, 3, 5), (23, 17, 15), (41, 31, 17)])
def test_blur_matches_ndimage(shape):
    from openscene_amd import ops
    noise = np.random.default_rng(sum(shape)).standard_normal(shape + (3,)).astype(np.float32)
    got = ops.elastic_blur(torch.from_numpy(noise).to(dev())).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), ref_blur(noise).view(np.uint32))


def test_bbox():
    from openscene_amd import ops
    x = room(100003, seed=3)
    got = ops.bbox(torch.from_numpy(x).to(dev())).cpu().numpy()
    assert np.array_equal(got, np.concatenate([x.min(0), x.max(0)]))


@pytest.mark.parametrize("g,m", [(0.2, 0.4), (0.8, 1.6)])
def test_elastic_distort_matches_scipy_on_a_room(g, m):
    from openscene_amd import ops
    x = room()
    np.random.seed(11)
    want = ref_field(x, g, m)
    np.random.seed(11)
    got, box = ops.elastic_distort(torch.from_numpy(x).to(dev()), g, m, return_bbox=True)
    got = got.cpu().numpy()
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), int((got != want).sum())
    assert np.array_equal(box.cpu().numpy(), np.concatenate([want.min(0), want.max(0)]))


@pytest.mark.parametrize("g,m", [(0.2, 0.4), (0.8, 1.6)])
def test_elastic_apply_out_of_grid_points(g, m):
    """A grid over the middle of the room: points beyond either end of an axis get no displacement (fill_value=0), points
    exactly on nodes and on the last node interpolate like scipy."""
    from openscene_amd import ops
    x = room()
    lo, hi = np.quantile(x, 0.2, 0), np.quantile(x, 0.8, 0)
    nd = ((hi - lo) // g).astype(int) + 3
    ax = [np.linspace(a, b, k) for a, b, k in zip(lo - g, lo + g * (nd - 2), nd)]
    x[:3000] = np.stack([a[np.random.default_rng(d).integers(0, k, 3000)] for d, (a, k) in enumerate(zip(ax, nd))], 1)
    x[3000:3100] = [a[-1] for a in ax]
    noise = ref_blur(np.random.default_rng(1).standard_normal((*nd, 3)).astype(np.float32))
    want = x + RegularGridInterpolator(ax, noise, bounds_error=0, fill_value=0)(x) * m
    out, box = ops.elastic_apply(torch.from_numpy(x).to(dev()), torch.from_numpy(noise).to(dev()), ax, m)
    got = out.cpu().numpy()
    outside = np.zeros(len(x), bool)
    for d in range(3):
        outside |= (x[:, d] < ax[d][0]) | (x[:, d] > ax[d][-1])
    assert 0.3 < outside.mean() < 0.9
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), int((got != want).sum())
    assert np.array_equal(got[outside], x[outside])
    assert np.array_equal(box.cpu().numpy(), np.concatenate([want.min(0), want.max(0)]))


def test_two_runs_are_identical(golden_dir, tmp_path):
    from openscene_amd.loader import TrainAugmentation
    x = torch.from_numpy(room(200000, seed=8)).to(dev())
    runs = []
    for _ in range(2):
        np.random.seed(4)
        random.seed(4)
        runs.append(TrainAugmentation().prevoxel_apply(x))
    assert torch.equal(runs[0], runs[1]) and not torch.equal(runs[0], x)
    d = plc.load(golden_dir)
    plc.write_scenes(d, tmp_path)
    a, b = (plc.run(d, tmp_path, dev(), plc.CASES[1]) for _ in range(2))
    assert all(torch.equal(u, v) for u, v in zip(a, b))


def test_error_paths():
    from openscene_amd import _lib, ops
    x = torch.from_numpy(room(1000)).to(dev())
    with pytest.raises(TypeError):
        ops.elastic_distort(x.float(), 0.2, 0.4)
    with pytest.raises(ValueError):
        ops.elastic_distort(x.t().contiguous().t(), 0.2, 0.4)
    with pytest.raises(ValueError):
        ops.bbox(x[:, :2])
    empty = torch.zeros((0, 3), dtype=torch.float64, device=dev())
    with pytest.raises(_lib.OpenSceneAmdError, match="empty"):
        ops.bbox(empty)
    with pytest.raises(_lib.OpenSceneAmdError, match="empty"):
        ops.elastic_distort(empty, 0.2, 0.4)
    noise = torch.zeros((3, 3, 3, 3), dtype=torch.float32, device=dev())
    with pytest.raises(_lib.OpenSceneAmdError, match="empty"):
        ops.elastic_apply(empty, noise, [np.arange(3.0)] * 3, 0.4)
    with pytest.raises(ValueError):
        ops.elastic_apply(x, noise, [np.arange(4.0)] * 3, 0.4)
    with pytest.raises(_lib.OpenSceneAmdError, match="2 nodes"):
        ops.elastic_apply(x, torch.zeros((1, 3, 3, 3), dtype=torch.float32, device=dev()), [np.arange(1.0)] + [np.arange(3.0)] * 2, 0.4)
