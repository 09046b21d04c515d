"""openscene_amd.render on the device against tests/render_reference.py: the z-buffer BITWISE equal to the numpy reference on
scenes whose projection is exact in float64 (no order of summation can matter) and on a general scene (the np.matmul the
fusion projection is already held to), consistent with the shipped projection kernel, the shading bit for bit in every
mode, and end to end: a search's heat column over rendered views, and the rendered depth stopping the bleed through a wall."""
import numpy as np
import pytest
import torch

import regions_reference as rr
import render_reference as rf
from openscene_amd import render as R

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda", 0)


def splat_case(c):
    from openscene_amd import ops
    xyz = torch.from_numpy(np.ascontiguousarray(c["coords"], dtype=np.float64).reshape(-1, 3)).to(dev())
    z = ops.render_splat(xyz, c["w2c"], c["k4"], c["image_hw"], radius=c["radius"], max_px=c["max_px"], near=c["near"])
    again = ops.render_splat(xyz, c["w2c"], c["k4"], c["image_hw"], radius=c["radius"], max_px=c["max_px"], near=c["near"])
    assert z.dtype == torch.int64 and tuple(z.shape) == (len(c["w2c"]),) + tuple(c["image_hw"])
    assert torch.equal(z, again)                                             # two calls, the same bits
    return rf.as_u64(z)


# ---------------------------------------------------------------------------------------------------- splat
@pytest.mark.parametrize("name", rf.exact_case_names())
def test_zbuf_bitwise_on_exact_arithmetic_cases(name):
    c = rf.exact_cases()[name]
    got = splat_case(c)
    want = rf.splat(c["coords"], c["w2c"], c["k4"], c["image_hw"], c["radius"], c["max_px"], c["near"])
    print("%s: %d of %d pixels drawn, %d differ" % (name, int((want != rf.BACKGROUND_KEY).sum()), want.size, int((got != want).sum())))
    assert np.array_equal(got, want)
    if name in ("n0", "nothing_drawn"):
        assert (got == rf.BACKGROUND_KEY).all()


RADIUS = 0.2                     # metres: discs of 1 and 2 pixels in a 64 x 48 view of the 5 m box


def random_views():
    s = rf.random_scene()
    return s, R.Cameras.orbit(s["xyz"], 3, image_hw=(48, 64))


def test_zbuf_bitwise_on_random_poses():
    s, cams = random_views()
    c = {"coords": s["xyz"], "w2c": cams.world_to_camera, "k4": cams.intrinsic, "image_hw": cams.image_hw, "radius": RADIUS, "max_px": 4,
         "near": 0.05}
    got = splat_case(c)
    want = rf.splat(s["xyz"], cams.world_to_camera, cams.intrinsic, cams.image_hw, RADIUS, 4, 0.05)
    print("random poses: %d pixels drawn, %d differ" % (int((want != rf.BACKGROUND_KEY).sum()), int((got != want).sum())))
    radii = np.rint(RADIUS * cams.intrinsic[0][0] / rf.project(cams.world_to_camera[0], cams.intrinsic[0], s["xyz"])[0])
    assert set(radii.tolist()) >= {1.0, 2.0}                            # footprints of several sizes
    assert (want != rf.BACKGROUND_KEY).sum() > 2000
    assert np.array_equal(got, want)


@pytest.mark.parametrize("radius", [0.0, RADIUS])
def test_centre_pixel_is_the_shipped_projection_kernels(radius):
    """For every point ops.fusion_project(depth=None) marks visible, the key at its centre pixel is <= the point's own key."""
    from openscene_amd import ops
    s, cams = random_views()
    xyz = torch.from_numpy(s["xyz"]).to(dev())
    near = 1e-3
    z = rf.as_u64(ops.render_splat(xyz, cams.world_to_camera, cams.intrinsic, cams.image_hw, radius=radius, max_px=4, near=near))
    for v in range(len(cams)):
        m = ops.fusion_project(xyz, cams.world_to_camera[v], cams.intrinsic[v], None, cams.image_hw, 0, 0.25).cpu().numpy()
        p2 = rf.project(cams.world_to_camera[v], cams.intrinsic[v], s["xyz"])[0]
        vis = np.nonzero(m[:, 2] == 1)[0]
        assert len(vis) > 1000 and (p2[vis] >= near).all()                   # (every visible point is also drawn)
        at_centre = z[v][m[vis, 0], m[vis, 1]]
        own = rf.keys_of(p2[vis], vis)
        assert (at_centre <= own).all()
        assert (at_centre == own).sum() > 20                                 # and some own their centre


# ---------------------------------------------------------------------------------------------------- shade
def shade_inputs():
    s = rf.random_scene(300, 7)
    z = rf.synthetic_zbuf(300)
    return s, z, torch.from_numpy(z.view(np.int64)).to(dev())


def assert_shade(got, want):
    pid, depth, rgb = got
    assert pid.dtype == torch.int32 and depth.dtype == torch.float32
    assert np.array_equal(pid.cpu().numpy(), want[0])
    assert np.array_equal(depth.cpu().numpy().view(np.uint32), want[1].view(np.uint32))
    if want[2] is None:
        assert rgb is None
    else:
        assert rgb.dtype == torch.uint8 and np.array_equal(rgb.cpu().numpy(), want[2])


def test_shade_ids_depth_colours_and_labels():
    from openscene_amd import ops
    s, z, zd = shade_inputs()
    n = 300
    assert_shade(ops.render_shade(zd, n), rf.shade(z, n))
    rgb = torch.from_numpy(s["rgb"]).to(dev())
    assert_shade(ops.render_shade(zd, n, "colors", colors=rgb, background=(1, 2, 3)), rf.shade(z, n, "colors", colors=s["rgb"], background=(1, 2, 3)))
    pal = R.palette(7)
    assert (s["labels"] == -1).any() and (s["labels"] == 7).any()             # outside the palette on both sides
    for dtype in (torch.int64, torch.int32):
        lab = torch.from_numpy(s["labels"]).to(dtype).to(dev())
        got = ops.render_shade(zd, n, "labels", values=lab, table=pal.to(dev()), other=(250, 251, 252), background=(9, 9, 9))
        assert_shade(got, rf.shade(z, n, "labels", values=s["labels"], table=pal.numpy(), other=(250, 251, 252), background=(9, 9, 9)))
    # a z-buffer drawn from more points than the arrays hold: the ids beyond them are never dereferenced
    assert_shade(ops.render_shade(zd, 100, "colors", colors=rgb[:100].contiguous()), rf.shade(z, 100, "colors", colors=s["rgb"][:100]))
    # an all-background image, and no pixels at all
    empty = np.full((1, 5, 7), rf.BACKGROUND_KEY, dtype=np.uint64)
    got = ops.render_shade(torch.from_numpy(empty.view(np.int64)).to(dev()), n, "colors", colors=rgb, background=(4, 5, 6))
    assert_shade(got, rf.shade(empty, n, "colors", colors=s["rgb"], background=(4, 5, 6)))
    assert (got[0] == -1).all() and (got[1] == 0).all() and got[2].reshape(-1, 3).unique(dim=0).tolist() == [[4, 5, 6]]
    none = ops.render_shade(torch.empty((0, 4, 4), dtype=torch.int64, device=dev()), n, "colors", colors=rgb)
    assert none[2].shape == (0, 4, 4, 3)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("with_base", [False, True])
def test_shade_heat_through_the_stride(dtype, with_base):
    from openscene_amd import ops
    s, z, zd = shade_inputs()
    n = 300
    heat = torch.from_numpy(s["heat"]).to(dtype)                              # [n, 5]; column 3 holds NaN, +-inf, values at and beyond lo / hi
    col = heat[:, 3].float().numpy()
    lo, hi = 0.25, 0.75
    assert np.isnan(col).any() and np.isposinf(col).any() and np.isneginf(col).any() and (col < lo).any() and (col > hi).any()
    assert (col == lo).any() and (col == hi).any()
    seen = col[rf.shade(z, n)[0][rf.shade(z, n)[0] >= 0]]                     # every kind of value is on some pixel
    assert np.isnan(seen).any() and np.isinf(seen).any() and (seen < lo).any() and (seen > hi).any()
    lut = R.default_lut()
    base = s["rgb"] if with_base else None
    hd = heat.to(dev())
    got = ops.render_shade(zd, n, "heat", values=hd, column=3, table=lut.to(dev()), lo=lo, hi=hi,
                           colors=None if base is None else torch.from_numpy(base).to(dev()), other=(255, 255, 255))
    want = rf.shade(z, n, "heat", colors=base, values=heat[:, 3].numpy(), table=lut.numpy(), lo=lo, hi=hi, other=(255, 255, 255))
    assert_shade(got, want)
    # the same column as a vector of its own, and an uneven range whose fp32 quotient rounds
    one = ops.render_shade(zd, n, "heat", values=hd[:, 3].contiguous(), table=lut.to(dev()), lo=lo, hi=hi,
                           colors=None if base is None else torch.from_numpy(base).to(dev()), other=(255, 255, 255))
    assert torch.equal(one[2], got[2])
    for q in (0, 4):
        got = ops.render_shade(zd, n, "heat", values=hd, column=q, table=lut.to(dev()), lo=0.1, hi=0.8)
        assert_shade(got, rf.shade(z, n, "heat", values=heat[:, q].numpy(), table=lut.numpy(), lo=0.1, hi=0.8))


# ---------------------------------------------------------------------------------------------------- end to end
def test_search_heat_column_over_rendered_views():
    from openscene_amd import search as S
    p = rr.planted()
    bank = S.FeatureBank(rr.PLANT_DIM, dev())
    for i, f in enumerate(p["feats"]):
        bank.add_scene("scene%d" % i, f.to(dev()))
    protos = torch.nn.functional.normalize(p["protos"], dim=1).half()
    res = S.search(bank, protos[:2], k=4, return_heat=True, negatives=protos[2:])
    scene, q = 1, 1
    xyz = p["xyz"][scene].double()
    n = xyz.shape[0]
    gen = torch.Generator().manual_seed(1)
    rgb = torch.randint(0, 256, (n, 3), generator=gen, dtype=torch.uint8)
    cams = R.Cameras.orbit(xyz, 2, image_hw=(48, 64))
    raster = R.rasterize(xyz.to(dev()), cams, radius=0.02, max_px=4)
    want_z = rf.splat(xyz.numpy(), cams.world_to_camera, cams.intrinsic, cams.image_hw, 0.02, 4, 0.05)
    assert np.array_equal(rf.as_u64(raster.zbuf), want_z)
    img = res.render(raster, scene, q, base=rgb)
    column = res.scene_heat(scene)[:, q].cpu().numpy()                        # the device's own heat column
    want = rf.shade(want_z, n, "heat", colors=rgb.numpy(), values=column, table=R.default_lut().numpy(), lo=0.5, hi=1.0)
    assert img.dtype == torch.uint8 and tuple(img.shape) == (2, 48, 64, 3) and np.array_equal(img.cpu().numpy(), want[2])
    assert np.array_equal(raster.point_id.cpu().numpy(), want[0])
    hit = column[want[0][want[0] >= 0]] >= 0.5
    assert hit.any() and (~hit).any()                                         # the picture shows hits and the base


def test_two_walls_on_the_device():
    rf.check_two_walls(*rf.two_wall_views(dev()))
