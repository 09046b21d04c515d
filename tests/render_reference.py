"""TEST INFRASTRUCTURE ONLY -- numpy restatement of the scene renderer (csrc/render.hip) and the builders of its test cases.

* ``project``: the projection of oracle.fusion.compute_mapping (the np.matmul formulation tests/test_fusion.py holds the
  device projection to, bit for bit), returning the depth and the rounded pixel instead of the mapping.
* ``splat``: the z-buffer by np.minimum.at on uint64 keys, one footprint offset at a time.
* ``shade``: point ids, depths and the three colour modes in float32 / integer numpy.
* ``render_splat`` / ``render_shade``: stand-ins with the signatures of the ops wrappers (CPU tensors), for the tests of the
  host code.
* ``exact_cases``: scenes whose projection is exact in float64 (axis-permutation poses with dyadic translations, coordinates
  on a 1/1024 grid, power-of-two focal lengths): no order of summation can change a bit.
"""
import functools

import numpy as np
import torch

BACKGROUND_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)


# ------------------------------------------------------------------------------------------------------ the two passes
def project(world_to_camera, k4, coords):
    """-> (p2, ur, vr) float64 [n]: oracle.fusion.compute_mapping's arithmetic up to the rounding."""
    n = coords.shape[0]
    coords_new = np.concatenate([coords, np.ones([n, 1])], axis=1).T
    p = np.matmul(world_to_camera, coords_new)
    with np.errstate(all="ignore"):
        u = (p[0] * k4[0]) / p[2] + k4[2]
        v = (p[1] * k4[1]) / p[2] + k4[3]
        return p[2].copy(), np.round(u), np.round(v)


def keys_of(p2, index):
    """(bits of float32(p2) << 32) | index, uint64."""
    with np.errstate(all="ignore"):
        bits = np.asarray(p2, dtype=np.float64).astype(np.float32).view(np.uint32).astype(np.uint64)
    return (bits << np.uint64(32)) | np.asarray(index).astype(np.uint64)


def splat(coords, world_to_camera, k4, image_hw, radius, max_px, near):
    """-> uint64 [V, H, W]"""
    coords = np.asarray(coords, dtype=np.float64).reshape(-1, 3)
    world_to_camera = np.asarray(world_to_camera, dtype=np.float64).reshape(-1, 4, 4)
    k4 = np.asarray(k4, dtype=np.float64).reshape(-1, 4)
    H, W = image_hw
    V, n = world_to_camera.shape[0], coords.shape[0]
    z = np.full((V, H * W), BACKGROUND_KEY, dtype=np.uint64)
    for v in range(V):
        p2, ur, vr = project(world_to_camera[v], k4[v], coords)
        with np.errstate(all="ignore"):
            zf = p2.astype(np.float32)
            ok = (p2 >= near) & ~np.isinf(zf) & (np.abs(ur) < 2.0 ** 30) & (np.abs(vr) < 2.0 ** 30)
            if radius == 0:
                r = np.zeros(n, dtype=np.int64)
            else:
                rr = np.rint((radius * k4[v][0]) / p2)
                rr = np.where(rr >= max_px, float(max_px), np.where(rr > 0, rr, 0.0))          # (NaN -> 0)
                r = np.where(ok, rr, 0.0).astype(np.int64)
        idx = np.nonzero(ok)[0]
        if idx.size == 0:
            continue
        key = keys_of(p2[idx], idx)
        cu, cv, r = ur[idx].astype(np.int64), vr[idx].astype(np.int64), r[idx]
        top = int(r.max())
        for dy in range(-top, top + 1):
            for dx in range(-top, top + 1):
                x, y = cu + dx, cv + dy
                m = (dx * dx + dy * dy <= r * r) & (x >= 0) & (x < W) & (y >= 0) & (y < H)
                if m.any():
                    np.minimum.at(z[v], y[m] * W + x[m], key[m])
    return z.reshape(V, H, W)


def _rgb(c):
    return np.array([int(x) for x in c], dtype=np.uint8)


def shade(zbuf, n, mode=None, colors=None, values=None, table=None, lo=0.0, hi=1.0, other=(255, 0, 255), background=(0, 0, 0)):
    """zbuf uint64 [...]; values: the [n] vector (labels, or the heat column).  -> (point_id int32, depth float32, rgb or None)"""
    z = np.asarray(zbuf, dtype=np.uint64)
    bg = z == BACKGROUND_KEY
    ids = (z & np.uint64(0xFFFFFFFF)).astype(np.int64)
    point_id = np.where(bg, -1, ids).astype(np.int32)
    depth = np.where(bg, np.float32(0), (z >> np.uint64(32)).astype(np.uint32).view(np.float32)).astype(np.float32)
    if mode is None:
        return point_id, depth, None
    rgb = np.empty(z.shape + (3,), dtype=np.uint8)
    rgb[...] = _rgb(other)
    fg = ~bg & (ids < n)
    i = ids[fg]
    if mode == "colors":
        rgb[fg] = colors[i]
    elif mode == "labels":
        lab = np.asarray(values)[i].astype(np.int64)
        good = (lab >= 0) & (lab < table.shape[0])
        out = np.tile(_rgb(other), (i.size, 1))
        out[good] = table[lab[good]]
        rgb[fg] = out
    elif mode == "heat":
        h = np.asarray(values)[i].astype(np.float32)
        lo32, hi32 = np.float32(lo), np.float32(hi)
        with np.errstate(all="ignore"):
            t = (h - lo32) / (hi32 - lo32)
            s = np.rint(t * np.float32(255))
            k = np.where(s >= 255, 255, np.where(s > 0, s, 0)).astype(np.int64)
        out = table[k]
        below = h < lo32
        out[below] = colors[i][below] if colors is not None else table[0]
        out[np.isnan(h)] = _rgb(other)
        rgb[fg] = out
    else:
        raise ValueError(mode)
    rgb[bg] = _rgb(background)
    return point_id, depth, rgb


# ------------------------------------------------------------------------------------------------------ stand-ins for ops.*
def as_u64(zbuf):
    """The uint64 numpy view of a z-buffer tensor (int64, any device)."""
    return zbuf.detach().cpu().numpy().view(np.uint64)


def render_splat(coords3, world_to_camera, intrinsics, image_hw, radius=0.02, max_px=4, near=0.05):
    z = splat(coords3.numpy(), world_to_camera, intrinsics, (int(image_hw[0]), int(image_hw[1])), float(radius), int(max_px), float(near))
    return torch.from_numpy(z.view(np.int64))


def render_shade(zbuf, n, mode=None, colors=None, values=None, column=0, table=None, lo=0.0, hi=1.0, other=(255, 0, 255),
                 background=(0, 0, 0)):
    if values is not None:
        values = values.numpy() if values.dim() == 1 else values.numpy()[:, column]
    pid, dep, rgb = shade(as_u64(zbuf), n, mode, None if colors is None else colors.numpy(), values,
                          None if table is None else table.numpy(), lo, hi, other, background)
    return torch.from_numpy(pid), torch.from_numpy(dep), None if rgb is None else torch.from_numpy(rgb)


# ------------------------------------------------------------------------------------------------------ exact cases
FX = 64.0                    # a power of two: p * fx is exact
H0, W0 = 48, 64
K0 = (FX, FX, 32.0, 24.0)


def _pose(perm, signs, t):
    """world_to_camera whose rotation is an axis permutation with sign flips and whose translation is dyadic."""
    m = np.zeros((4, 4))
    for row, (axis, s) in enumerate(zip(perm, signs)):
        m[row, axis] = s
    m[:3, 3] = t
    m[3, 3] = 1.0
    return m


POSES = (_pose((0, 1, 2), (1, 1, 1), (0.0, 0.0, 0.0)),
         _pose((1, 2, 0), (1, -1, 1), (0.25, -0.5, 1.0)),
         _pose((2, 0, 1), (-1, 1, -1), (-0.125, 0.75, 3.0)))


def world_of(cam, pose):
    """The world point a permutation pose maps to the camera-space point `cam` (exact)."""
    r, t = pose[:3, :3], pose[:3, 3]
    with np.errstate(invalid="ignore"):
        return (np.asarray(cam, dtype=np.float64) - t) @ r


def at_pixel(u, v, z, k4=K0):
    """The camera-space point that projects to (u, v) at depth z; the choice must be exact."""
    x, y = (u - k4[2]) * z / k4[0], (v - k4[3]) * z / k4[1]
    assert (x * k4[0]) / z + k4[2] == u and (y * k4[1]) / z + k4[3] == v
    return (x, y, z)


def _case(cam_points, pose=0, image_hw=(H0, W0), radius=0.0, max_px=4, near=0.05, k4=K0):
    pts = np.asarray(cam_points, dtype=np.float64).reshape(-1, 3)
    poses = POSES[pose:pose + 1] if isinstance(pose, int) else [POSES[i] for i in pose]
    coords = world_of(pts, poses[0]) if len(pts) else np.zeros((0, 3))
    return {"coords": coords, "w2c": np.stack(poses), "k4": np.tile(np.asarray(k4, dtype=np.float64), (len(poses), 1)),
            "image_hw": image_hw, "radius": radius, "max_px": max_px, "near": near}


R3 = 3.0 / 32.0              # radius * FX = 6: r = rint(6 / z) -- 3 pixels at z = 2


@functools.lru_cache(maxsize=None)
def exact_cases():
    rng = np.random.default_rng(5)
    c = {}
    c["n0"] = _case([])
    c["n1_r0"] = _case([at_pixel(10.0, 7.0, 2.0)], pose=1)
    # u = k + 0.5 exactly: round half to even sends 2.5 -> 2, 3.5 -> 4 (and the rows 6.5 -> 6, 7.5 -> 8)
    c["half_pixel_ties"] = _case([at_pixel(2.5, 6.5, 2.0), at_pixel(3.5, 7.5, 2.0), at_pixel(20.5, 11.5, 4.0), at_pixel(21.5, 10.5, 4.0)], pose=2)
    c["equal_depth"] = _case([at_pixel(5.0, 5.0, 4.0), at_pixel(9.0, 9.0, 2.0), at_pixel(9.0, 9.0, 2.0), at_pixel(5.0, 5.0, 2.0)], pose=1)
    # 2 + 2^-30 and 2 differ in float64 and round to one float32: the LOWER index wins although it is farther
    c["equal_float32_depth"] = _case([at_pixel(32.0, 24.0, 2.0 + 2.0 ** -30), at_pixel(32.0, 24.0, 2.0)])
    edge = [(0.0, 20.0), (W0 - 1.0, 20.0), (30.0, 0.0), (30.0, H0 - 1.0), (0.0, 0.0), (W0 - 1.0, H0 - 1.0), (0.0, H0 - 1.0), (W0 - 1.0, 0.0)]
    c["clipped_at_borders"] = _case([at_pixel(u, v, 2.0) for u, v in edge], pose=2, radius=R3)
    outside = [(-2.0, 10.0), (W0 + 1.0, 30.0), (20.0, -3.0), (40.0, H0 + 2.0), (-2.0, -2.0), (-10.0, 20.0), (20.0, H0 + 3.0)]     # the last two: nothing, by far and by one row
    c["centre_outside"] = _case([at_pixel(u, v, 2.0) for u, v in outside], pose=1, radius=R3)
    bad = [(0.0, 0.0, 1.0 / 64), (0.0, 0.0, -2.0), (0.0, 0.0, 0.0), (np.nan, 0.0, 2.0), (0.0, np.inf, 2.0), (0.0, 0.0, np.inf),
           (0.0, 0.0, -np.inf), (0.0, 0.0, np.nan), (0.0, 0.0, 1e300), (2.0 ** 40, 0.0, 1.0)]
    c["nothing_drawn"] = _case(bad, radius=R3, near=1.0 / 32)
    c["max_px_clamp"] = _case([at_pixel(32.0, 24.0, 1.0 / 16), at_pixel(5.0, 40.0, 2.0)], pose=1, radius=R3, max_px=5, near=1.0 / 64)
    ladder = [16.0, 8.0, 4.0, 2.0, 1.5, 1.25, 1.0]                      # r = rint(6 / z) = 0, 1, 2 (tie to even), 3, 4, 5, 6
    c["radius_ladder"] = _case([at_pixel(4.0 + 9.0 * i, 8.0 + 5.0 * i, z) for i, z in enumerate(ladder)]
                               + [at_pixel(30.0, 24.0, z) for z in ladder], pose=2, radius=R3, max_px=6)
    grid = rng.integers(-3072, 3072, size=(4096, 3)) / 1024.0
    grid[:, 2] = rng.integers(256, 8192, size=4096) / 1024.0
    c["contention_8x8"] = _case(grid, pose=0, image_hw=(8, 8), radius=1.0 / 8, max_px=2, k4=(4.0, 4.0, 3.5, 4.0))
    cloud = rng.integers(-2048, 2048, size=(600, 3)) / 1024.0
    c["three_views_37x53"] = dict(_case([], pose=(0, 1, 2), image_hw=(37, 53), radius=1.0 / 16, max_px=3, k4=(32.0, 32.0, 26.0, 18.5)),
                                  coords=cloud)
    return c


def exact_case_names():
    return list(exact_cases())


def expected_radii(case):
    """The pixel radius of every point of a one-view case (the reference's own rule, for the case checks)."""
    p2, _, _ = project(case["w2c"][0], case["k4"][0], case["coords"])
    with np.errstate(all="ignore"):
        rr = np.rint((case["radius"] * case["k4"][0][0]) / p2)
    return np.where(rr >= case["max_px"], case["max_px"], np.where(rr > 0, rr, 0)).astype(int)


# ------------------------------------------------------------------------------------------------------ general scenes
@functools.lru_cache(maxsize=None)
def random_scene(n=5000, seed=11):
    """A box of points with colours, labels and heat columns (special values planted in column 3)."""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform((-2.0, -1.5, 0.0), (2.0, 1.5, 2.5), size=(n, 3))
    rgb = rng.integers(0, 256, size=(n, 3), dtype=np.uint8)
    labels = rng.integers(-1, 8, size=n)                                  # -1 and 7 = C are outside a palette of 7
    heat = rng.uniform(-0.2, 1.2, size=(n, 5)).astype(np.float32)
    special = np.array([np.nan, np.inf, -np.inf, 0.25, 0.75, 0.2499, 0.7501, 0.5, -1.0, 2.0], dtype=np.float32)
    reps = min(40, n // 20)
    heat[:, 3][rng.permutation(n)[:10 * reps]] = np.tile(special, reps)
    return {"xyz": xyz, "rgb": rgb, "labels": labels, "heat": heat}


@functools.lru_cache(maxsize=None)
def synthetic_zbuf(n=300, shape=(2, 16, 20), seed=3, background=0.3):
    """A z-buffer in which every point of 0 .. n-1 owns at least one pixel when there is room, with background holes."""
    rng = np.random.default_rng(seed)
    size = int(np.prod(shape))
    ids = rng.integers(0, n, size=size)
    ids[:min(n, size)] = np.arange(min(n, size))
    rng.shuffle(ids)
    z = keys_of(rng.uniform(0.1, 9.0, size=size), ids)
    z[rng.random(size) < background] = BACKGROUND_KEY
    return z.reshape(shape)


WALL_NEAR, WALL_FAR = 2.0, 3.0


@functools.lru_cache(maxsize=None)
def two_walls():
    """A camera at the origin looking along +z (identity pose) at a near wall (z = 2, 2 cm samples: denser than a pixel) with
    a far wall 1 m behind it (z = 3, 5 cm samples, wider than the near one).  `behind`: the far points whose ray crosses the
    near wall at least 5 cm inside its rim."""
    xs, ys = np.arange(-0.6, 0.6001, 0.02), np.arange(-0.4, 0.4001, 0.02)
    near = np.stack(np.meshgrid(xs, ys, indexing="ij"), -1).reshape(-1, 2)
    xf, yf = np.arange(-1.4, 1.4001, 0.05), np.arange(-1.0, 1.0001, 0.05)
    far = np.stack(np.meshgrid(xf, yf, indexing="ij"), -1).reshape(-1, 2)
    xyz = np.concatenate([np.concatenate([near, np.full((len(near), 1), WALL_NEAR)], 1),
                          np.concatenate([far, np.full((len(far), 1), WALL_FAR)], 1)])
    ray = far * (WALL_NEAR / WALL_FAR)
    behind = np.nonzero((np.abs(ray[:, 0]) <= 0.55) & (np.abs(ray[:, 1]) <= 0.35))[0] + len(near)
    return {"xyz": xyz, "n_near": len(near), "behind": behind, "camera_to_world": np.eye(4), "image_hw": (48, 64), "fov_deg": 60.0,
            "radius": 0.02}


def two_wall_views(device):
    """The two walls through rasterize and PointCloudToImageMapper on `device`: without a depth image, and against the rendered one."""
    from openscene_amd import render as R
    from openscene_amd.fusion import PointCloudToImageMapper
    w = two_walls()
    cams = R.Cameras(w["camera_to_world"][None], (32.0 / np.tan(np.radians(30.0)),) * 2 + (31.5, 23.5), w["image_hw"])
    raster = R.rasterize(w["xyz"], cams, radius=w["radius"], max_px=4, near=0.05, device=device)
    mapper = PointCloudToImageMapper((64, 48), visibility_threshold=0.25, device=device)
    k = cams.intrinsic_matrix(0)
    free = mapper.compute_mapping(w["camera_to_world"], w["xyz"], None, k)
    held = mapper.compute_mapping(w["camera_to_world"], w["xyz"], raster.fusion_depth(0), k)
    return w, cams, raster, free.cpu().numpy(), held.cpu().numpy()


def check_two_walls(w, cams, raster, free, held):
    pid, depth = raster.point_id.cpu().numpy()[0], raster.depth.cpu().numpy()[0]
    # the near wall leaves no hole: every pixel inside its projected rim (5 cm in) belongs to one of its points
    fx, _, cx, cy = cams.intrinsic[0]
    us = np.arange(int(np.ceil(cx - 0.55 * fx / 2)), int(np.floor(cx + 0.55 * fx / 2)) + 1)
    vs = np.arange(int(np.ceil(cy - 0.35 * fx / 2)), int(np.floor(cy + 0.35 * fx / 2)) + 1)
    patch = pid[np.ix_(vs, us)]
    assert len(us) > 25 and len(vs) > 15 and (patch >= 0).all() and (patch < w["n_near"]).all()
    assert (depth[np.ix_(vs, us)] == np.float32(WALL_NEAR)).all()
    behind = w["behind"]
    assert len(behind) > 300
    assert (free[behind, 2] == 1).all()                                      # without a depth image they shine through the wall
    assert (held[behind, 2] == 0).all()                                      # against the rendered depth none of them does
    assert (held[:w["n_near"], 2] == free[:w["n_near"], 2]).all() and held[:w["n_near"], 2].sum() > 1000
    far_seen = np.nonzero(held[w["n_near"]:, 2] == 1)[0]
    assert len(far_seen) > 100                                               # the far wall beside the near one is still seen
