"""Host logic of openscene_amd.render WITHOUT a GPU: ops.render_splat / ops.render_shade / ops.fusion_project are replaced by
the stand-ins of tests/render_reference.py and tests/cpu_backend.py, so Cameras, rasterize, Raster, SearchResult.render and
save_png are the code under test; the wrappers' argument checks run as they are (they come before the device check).  The
reference's own invariants -- what tests/test_gpu_render.py relies on -- are checked here, on the same inputs."""
import os
import re
import struct
import zlib

import numpy as np
import pytest
import torch

import cpu_backend
import render_reference as rf
import search_contrast_reference as scr
import search_reference as sr
from openscene_amd import _lib
from openscene_amd import io as osn_io
from openscene_amd import ops
from openscene_amd import render as R
from openscene_amd import search as S
from openscene_amd.fusion import PointCloudToImageMapper

CPU = torch.device("cpu")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = {"osn_render_splat", "osn_render_shade"}
REAL_SPLAT, REAL_SHADE = ops.render_splat, ops.render_shade


@pytest.fixture(autouse=True)
def cpu_kernels(monkeypatch):
    for name, f in (("render_splat", rf.render_splat), ("render_shade", rf.render_shade), ("fusion_project", cpu_backend.fusion_project),
                    ("bank_append", sr.bank_append), ("bank_check", sr.bank_check), ("bank_search", scr.bank_search)):
        monkeypatch.setattr(ops, name, f)


# ---------------------------------------------------------------------------------------------------- the header
def test_the_header_declares_exactly_the_new_entries_the_prototypes_list():
    src = open(os.path.join(ROOT, "include", "openscene_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = {n for n in re.findall(r"\b(osn_[a-z0-9_]+)\s*\(", code) if n.startswith("osn_render_")}
    assert declared == NEW_ENTRIES == {n for n in _lib.PROTOTYPES if n.startswith("osn_render_")}
    block = src[src.index("csrc/render.hip"):src.index("int osn_render_splat(")]
    for word in ("all ones", "2^32 - 1", "atomic min", "lower point index", "csrc/project.h", "-1 background", "NaN gives `other`"):
        assert word in block, word
    for name in NEW_ENTRIES:                                                 # the argument counts agree
        decl = re.search(name + r"\s*\((.*?)\);", code, flags=re.S).group(1)
        assert len(decl.split(",")) == len(_lib.PROTOTYPES[name][1]), name
    assert "render.hip" in open(os.path.join(ROOT, "openscene_amd", "build.py")).read()
    # one projection body: both kernels' files include it and neither restates the chain
    csrc = os.path.join(ROOT, "openscene_amd", "csrc")
    for f in ("fusion.hip", "render.hip"):
        text = open(os.path.join(csrc, f)).read()
        assert '#include "project.h"' in text and "project_point(" in text and "__ddiv_rn(__dmul_rn(p[" not in text, f


# ---------------------------------------------------------------------------------------------------- argument checks
def test_render_splat_refuses_bad_arguments():
    xyz = torch.zeros((4, 3), dtype=torch.float64)
    w2c, k4 = np.eye(4)[None], np.array([[32.0, 32.0, 16.0, 12.0]])
    ok = dict(image_hw=(24, 32), radius=0.02, max_px=4, near=0.05)
    with pytest.raises(TypeError):
        REAL_SPLAT(xyz.float(), w2c, k4, **ok)
    with pytest.raises(ValueError):
        REAL_SPLAT(xyz.t().contiguous().t(), w2c, k4, **ok)                 # not contiguous
    with pytest.raises(ValueError):
        REAL_SPLAT(xyz[:, :2].contiguous(), w2c, k4, **ok)
    with pytest.raises(ValueError):
        REAL_SPLAT(xyz, np.eye(4), k4, **ok)
    with pytest.raises(ValueError):
        REAL_SPLAT(xyz, w2c, k4[0], **ok)
    for bad in (dict(image_hw=(0, 32)), dict(image_hw=(1 << 16, 1 << 15)), dict(radius=-0.1), dict(radius=float("nan")),
                dict(radius=float("inf")), dict(max_px=-1), dict(max_px=17), dict(near=0.0), dict(near=float("nan")), dict(near=float("inf"))):
        with pytest.raises(ValueError):
            REAL_SPLAT(xyz, w2c, k4, **dict(ok, **bad))
    with pytest.raises(_lib.OpenSceneAmdError):                              # every check passed: only the device is missing
        REAL_SPLAT(xyz, w2c, k4, **ok)


def test_render_shade_refuses_bad_arguments():
    z = torch.full((2, 3, 4), -1, dtype=torch.int64)
    n = 5
    rgb = torch.zeros((n, 3), dtype=torch.uint8)
    lut = torch.zeros((256, 3), dtype=torch.uint8)
    heat = torch.zeros((n, 4), dtype=torch.float16)
    labels = torch.zeros(n, dtype=torch.int64)
    with pytest.raises(TypeError):
        REAL_SHADE(z.int(), n)
    with pytest.raises(ValueError):
        REAL_SHADE(z.transpose(0, 1), n)
    with pytest.raises(ValueError):
        REAL_SHADE(z, -1)
    with pytest.raises(ValueError):
        REAL_SHADE(z, 1 << 31)
    with pytest.raises(ValueError):
        REAL_SHADE(z, n, "depth")
    with pytest.raises(TypeError):
        REAL_SHADE(z, n, "colors", colors=rgb.float())
    with pytest.raises(ValueError):
        REAL_SHADE(z, n, "colors", colors=rgb[:4])
    with pytest.raises(ValueError):
        REAL_SHADE(z, n, "labels", values=labels, table=rgb, colors=rgb)
    with pytest.raises(TypeError):
        REAL_SHADE(z, n, "labels", values=labels.float(), table=rgb)
    with pytest.raises(ValueError):
        REAL_SHADE(z, n, "labels", values=labels[:4], table=rgb)
    with pytest.raises(TypeError):
        REAL_SHADE(z, n, "heat", values=heat.double(), table=lut)
    with pytest.raises(ValueError):
        REAL_SHADE(z, n, "heat", values=heat, column=4, table=lut)
    with pytest.raises(ValueError):
        REAL_SHADE(z, n, "heat", values=heat, column=1, table=lut[:255])
    for lo, hi in ((1.0, 1.0), (1.0, 0.0), (float("nan"), 1.0), (0.0, float("inf")), (1.0, 1.0 + 1e-12)):
        with pytest.raises(ValueError):
            REAL_SHADE(z, n, "heat", values=heat, column=1, table=lut, lo=lo, hi=hi)
    with pytest.raises(ValueError):
        REAL_SHADE(z, n, "heat", values=heat, column=1, table=lut, other=(0, 0, 256))
    with pytest.raises(ValueError):
        REAL_SHADE(z, n, None, values=labels)
    with pytest.raises(_lib.OpenSceneAmdError):
        REAL_SHADE(z, n, "heat", values=heat, column=3, table=lut, colors=rgb, lo=0.5, hi=1.0)


# ---------------------------------------------------------------------------------------------------- cameras
def test_look_at_sends_the_target_to_the_image_centre():
    eyes = np.array([(3.0, 1.0, 2.0), (-2.0, 0.5, 0.3), (0.0, -4.0, 1.0)])
    targets = np.array([(0.0, 0.0, 0.5), (1.0, 1.0, 1.0), (0.2, 0.1, -0.3)])
    cams = R.Cameras.look_at(eyes, targets, fov_deg=70.0, image_hw=(48, 64))
    assert len(cams) == 3 and cams.image_hw == (48, 64)
    for v in range(3):
        p = cams.world_to_camera[v] @ np.append(targets[v], 1.0)
        fx, fy, cx, cy = cams.intrinsic[v]
        assert p[2] == pytest.approx(np.linalg.norm(targets[v] - eyes[v])) and (cx, cy) == (31.5, 23.5)
        assert abs(p[0] * fx / p[2]) < 1e-9 and abs(p[1] * fy / p[2]) < 1e-9        # on the principal point
        rot = cams.camera_to_world[v][:3, :3]
        assert np.allclose(rot.T @ rot, np.eye(3), atol=1e-12) and np.linalg.det(rot) == pytest.approx(1.0)
        assert rot[2, 1] < 0                                                         # the image's down is the world's down (z up)
        assert np.array_equal(cams.world_to_camera[v], np.linalg.inv(cams.camera_to_world[v]))
    assert fx == pytest.approx(32.0 / np.tan(np.radians(35.0))) and fx == fy
    with pytest.raises(ValueError):
        R.Cameras.look_at(eyes, eyes)
    with pytest.raises(ValueError):
        R.Cameras.look_at([(0.0, 0.0, 1.0)], [(0.0, 0.0, 0.0)])                       # along `up`
    with pytest.raises(ValueError):
        R.Cameras(np.eye(4)[None], (1.0, 1.0), (4, 4))


@pytest.mark.parametrize("hw,elev", [((48, 64), 30.0), ((64, 48), 60.0), ((37, 53), 0.0)])
def test_every_corner_of_the_box_is_inside_every_orbit_view(hw, elev):
    rng = np.random.default_rng(2)
    xyz = rng.uniform((-3.0, 1.0, 0.0), (5.0, 4.0, 2.5), size=(200, 3))
    cams = R.Cameras.orbit(torch.from_numpy(xyz), 7, elevation_deg=elev, image_hw=hw)
    lo, hi = xyz.min(0), xyz.max(0)
    corners = np.array([(x, y, z) for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
    eyes = cams.camera_to_world[:, :3, 3]
    assert np.allclose(np.linalg.norm(eyes - 0.5 * (lo + hi), axis=1), np.linalg.norm(eyes[0] - 0.5 * (lo + hi)))
    assert len({tuple(np.round(e, 9)) for e in eyes}) == 7
    for v in range(7):
        p2, ur, vr = rf.project(cams.world_to_camera[v], cams.intrinsic[v], corners)
        assert (p2 > 0).all() and (ur >= 0).all() and (ur < hw[1]).all() and (vr >= 0).all() and (vr < hw[0]).all()


# ---------------------------------------------------------------------------------------------------- the reference itself
def test_the_exact_cases_hold_what_the_gpu_tests_rely_on():
    cases = rf.exact_cases()
    bg = rf.BACKGROUND_KEY

    def run(name):
        c = cases[name]
        z = rf.splat(c["coords"], c["w2c"], c["k4"], c["image_hw"], c["radius"], c["max_px"], c["near"])
        return c, z, rf.shade(z, len(c["coords"]))[0]

    for name, c in cases.items():                                            # the construction: everything is dyadic
        assert np.array_equal(c["w2c"] * 1024, np.round(c["w2c"] * 1024)) and all(np.log2(k).is_integer() for k in c["k4"][:, :2].ravel())
    _, z, _ = run("n0")
    assert z.shape == (1, 48, 64) and (z == bg).all()
    _, z, pid = run("n1_r0")
    assert (z != bg).sum() == 1 and pid[0, 7, 10] == 0
    _, z, pid = run("half_pixel_ties")
    assert pid[0, 6, 2] == 0 and pid[0, 8, 4] == 1 and pid[0, 12, 20] == 2 and pid[0, 10, 22] == 3 and (z != bg).sum() == 4
    _, z, pid = run("equal_depth")
    assert pid[0, 9, 9] == 1 and pid[0, 5, 5] == 3 and (z != bg).sum() == 2
    c, z, pid = run("equal_float32_depth")
    p2 = rf.project(c["w2c"][0], c["k4"][0], c["coords"])[0]
    assert p2[0] > p2[1] and np.float32(p2[0]) == np.float32(p2[1]) and pid[0, 24, 32] == 0
    c, z, pid = run("clipped_at_borders")
    assert (rf.expected_radii(c) == 3).all()
    full = 29                                                                # pixels of a disc of radius 3
    counts = np.bincount(pid[pid >= 0], minlength=8)
    assert (counts[:4] < full).all() and (counts[:4] > full // 2).all() and (counts[4:] < full // 2).all() and (counts[4:] > 0).all()
    c, z, pid = run("centre_outside")
    counts = np.bincount(pid[pid >= 0], minlength=7)
    assert (counts[:5] > 0).all() and counts[5] == 0 and counts[6] == 0 and (counts[:4] < full // 2).all()
    _, z, _ = run("nothing_drawn")
    assert (z == bg).all()
    c, z, pid = run("max_px_clamp")
    assert rf.expected_radii(c).tolist() == [5, 3] and (pid == 0).sum() == 81 and (pid == 1).sum() == full
    c, z, pid = run("radius_ladder")
    assert rf.expected_radii(c)[:7].tolist() == [0, 1, 2, 3, 4, 5, 6]
    areas = [1, 5, 13, 29, 49, 81, 113]
    assert (pid == 13).sum() == 113 and pid[0, 24, 30] == 13                 # the nearest of the stacked points owns its whole disc
    assert [(pid == i).sum() <= a for i, a in enumerate(areas)] == [True] * 7 and (pid == 0).sum() == 1
    c, z, pid = run("contention_8x8")
    assert (z != bg).all() and len(c["coords"]) == 4096 and set(rf.expected_radii(c).tolist()) == {0, 1, 2}
    c, z, pid = run("three_views_37x53")
    assert z.shape == (3, 37, 53) and all((pid[v] >= 0).sum() > 100 for v in range(3))


def test_the_reference_projection_is_the_oracles():
    from oracle import fusion as of
    s = rf.random_scene()
    cams = R.Cameras.orbit(s["xyz"], 3, image_hw=(48, 64))
    for v in range(3):
        m = of.compute_mapping(None, s["xyz"], None, cams.intrinsic_matrix(v), (64, 48), world_to_camera=cams.world_to_camera[v])
        p2, ur, vr = rf.project(cams.world_to_camera[v], cams.intrinsic[v], s["xyz"])
        vis = m[:, 2] == 1
        assert vis.sum() > 1000
        assert np.array_equal(m[vis, 0], vr[vis].astype(np.int64)) and np.array_equal(m[vis, 1], ur[vis].astype(np.int64))
        assert np.array_equal(vis, (p2 > 0) & (ur >= 0) & (ur < 64) & (vr >= 0) & (vr < 48))


def test_rendered_depth_keeps_what_is_seen_and_equals_the_float32_depth():
    """(a) a point compute_mapping(depth=None) marks visible, and that owns its centre pixel, stays visible against the
    rendered depth; (c) the depth of a pixel is float32(p2) of its winner."""
    s = rf.random_scene()
    cams = R.Cameras.orbit(s["xyz"], 3, image_hw=(48, 64))
    raster = R.rasterize(s["xyz"], cams, radius=0.02, max_px=4, near=0.05, device="cpu")
    assert raster.point_id.shape == raster.depth.shape == (3, 48, 64) and raster.point_id.dtype == torch.int32
    mapper = PointCloudToImageMapper((64, 48), visibility_threshold=0.25, device="cpu")
    pid = raster.point_id.numpy()
    for v in range(3):
        k = cams.intrinsic_matrix(v)
        free = mapper.compute_mapping(cams.camera_to_world[v], s["xyz"], None, k).numpy()
        depth = raster.fusion_depth(v)
        assert depth.dtype == torch.float64 and tuple(depth.shape) == (48, 64)
        held = mapper.compute_mapping(cams.camera_to_world[v], s["xyz"], depth, k).numpy()
        vis = np.nonzero(free[:, 2] == 1)[0]
        owner = vis[pid[v][free[vis, 0], free[vis, 1]] == vis]
        assert len(owner) > 500 and (held[owner, 2] == 1).all() and np.array_equal(held[owner], free[owner])
        assert (held[:, 2] <= free[:, 2]).all() and held[:, 2].sum() < free[:, 2].sum()       # and some points are now hidden
        p2 = rf.project(cams.world_to_camera[v], cams.intrinsic[v], s["xyz"])[0]
        fg = pid[v] >= 0
        assert np.array_equal(raster.depth[v].numpy()[fg], p2[pid[v][fg]].astype(np.float32))
        assert (raster.depth[v].numpy()[~fg] == 0).all()


def test_two_walls_the_rendered_depth_stops_the_bleed():
    rf.check_two_walls(*rf.two_wall_views("cpu"))


# ---------------------------------------------------------------------------------------------------- shading front ends
def test_raster_pictures_and_palette():
    s = rf.random_scene()
    cams = R.Cameras.orbit(s["xyz"], 2, image_hw=(24, 32))
    raster = R.rasterize(s["xyz"], cams, device="cpu")
    z = rf.as_u64(raster.zbuf)
    rgb, labels, heat = torch.from_numpy(s["rgb"]), torch.from_numpy(s["labels"]), torch.from_numpy(s["heat"])
    pal = R.palette(7)
    assert pal.dtype == torch.uint8 and tuple(pal.shape) == (7, 3) and torch.equal(pal, R.palette(7)) and torch.equal(pal[:5], R.palette(5))
    assert len({tuple(c) for c in pal.tolist()}) == 7
    lut = R.default_lut()
    assert lut.dtype == torch.uint8 and tuple(lut.shape) == (256, 3) and len({tuple(c) for c in lut.tolist()}) > 200
    assert lut[0].tolist() == [0, 0, 96] and lut[255].tolist() == [224, 0, 0]
    n = len(s["xyz"])
    assert np.array_equal(raster.colors(rgb, background=(9, 8, 7)).numpy(), rf.shade(z, n, "colors", colors=s["rgb"], background=(9, 8, 7))[2])
    got = raster.labels(labels, pal, other=(1, 2, 3)).numpy()
    assert np.array_equal(got, rf.shade(z, n, "labels", values=s["labels"], table=pal.numpy(), other=(1, 2, 3))[2])
    assert got.shape == (2, 24, 32, 3) and got.dtype == np.uint8
    got = raster.heat(heat, 0.25, 0.75, base=rgb, column=3).numpy()
    assert np.array_equal(got, rf.shade(z, n, "heat", colors=s["rgb"], values=s["heat"][:, 3], table=lut.numpy(), lo=0.25, hi=0.75)[2])
    with pytest.raises(TypeError):
        R.rasterize(s["xyz"], None)
    with pytest.raises(ValueError):
        R.rasterize(s["xyz"][:, :2], cams, device="cpu")


def test_search_result_render_shades_the_strided_column(monkeypatch):
    s = rf.random_scene()
    n = len(s["xyz"])
    gen = torch.Generator().manual_seed(4)
    bank = S.FeatureBank(16, CPU)
    feats = [torch.randn(37, 16, generator=gen).half(), torch.randn(n, 16, generator=gen).half()]
    for i, f in enumerate(feats):
        bank.add_scene("s%d" % i, f)
    q = torch.nn.functional.normalize(torch.randn(5, 16, generator=gen), dim=1).half()
    cams = R.Cameras.orbit(s["xyz"], 2, image_hw=(24, 32))
    raster = R.rasterize(s["xyz"], cams, device="cpu")
    rgb = torch.from_numpy(s["rgb"])
    seen = {}
    real = ops.render_shade

    def spy(zbuf, n, mode=None, **kw):
        if mode == "heat":
            seen.update(kw)
        return real(zbuf, n, mode, **kw)
    monkeypatch.setattr(ops, "render_shade", spy)
    z = rf.as_u64(raster.zbuf)
    lut = R.default_lut().numpy()
    plain = S.search(bank, q, k=4, return_heat=True)
    with pytest.raises(ValueError):
        plain.render(raster, "s1", 2)                                        # plain scores: lo and hi are required
    img = plain.render(raster, "s1", 2, lo=0.1, hi=0.6, base=rgb)
    # the column is used in place: the [n, Q] rows of the scene, a view into the search's heat-map
    assert seen["column"] == 2 and seen["values"].data_ptr() == plain.heat[37:].data_ptr() and tuple(seen["values"].shape) == (n, 5)
    want = rf.shade(z, n, "heat", colors=s["rgb"], values=plain.heat[37:, 2].numpy(), table=lut, lo=0.1, hi=0.6)[2]
    assert np.array_equal(img.numpy(), want) and (want != want[0, 0, 0]).any()
    rel = S.search(bank, q[:2], k=4, return_heat=True, negatives=q[2:])
    img = rel.render(raster, 1, 1)
    assert (seen["lo"], seen["hi"]) == (0.5, 1.0)
    assert np.array_equal(img.numpy(), rf.shade(z, n, "heat", values=rel.heat[37:, 1].numpy(), table=lut, lo=0.5, hi=1.0)[2])
    with pytest.raises(IndexError):
        rel.render(raster, 1, 2)
    with pytest.raises(ValueError):
        rel.render(raster, 0, 1)                                             # another scene's points
    with pytest.raises(ValueError, match="without return_heat"):
        S.search(bank, q, k=4).render(raster, 1, 0, lo=0.0, hi=1.0)


# ---------------------------------------------------------------------------------------------------- PNG
def test_save_png_round_trip(tmp_path):
    rng = np.random.default_rng(0)
    for shape in ((5, 7, 3), (1, 1, 3), (48, 64, 3)):
        img = rng.integers(0, 256, size=shape, dtype=np.uint8)
        path = osn_io.save_png(str(tmp_path / "a.png"), torch.from_numpy(img))
        data = open(path, "rb").read()
        assert data[:8] == b"\x89PNG\r\n\x1a\n"
        pos, chunks = 8, []
        while pos < len(data):
            size, kind = struct.unpack(">I4s", data[pos:pos + 8])
            body = data[pos + 8:pos + 8 + size]
            assert struct.unpack(">I", data[pos + 8 + size:pos + 12 + size])[0] == zlib.crc32(kind + body) & 0xFFFFFFFF
            chunks.append((kind, body))
            pos += 12 + size
        assert [k for k, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
        assert struct.unpack(">IIBBBBB", chunks[0][1]) == (shape[1], shape[0], 8, 2, 0, 0, 0)
        raw = np.frombuffer(zlib.decompress(chunks[1][1]), dtype=np.uint8).reshape(shape[0], 1 + 3 * shape[1])
        assert (raw[:, 0] == 0).all() and np.array_equal(raw[:, 1:].reshape(shape), img)          # filter type 0: the bytes themselves
    for bad in (np.zeros((4, 4), np.uint8), np.zeros((4, 4, 4), np.uint8), np.zeros((4, 4, 3), np.float32), np.zeros((0, 4, 3), np.uint8)):
        with pytest.raises(ValueError):
            osn_io.save_png(str(tmp_path / "b.png"), bad)
