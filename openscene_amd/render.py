"""Scene views on the GPU: look at a result without leaving the device or the package.

The reference's headline is a picture -- the interactive demo that highlights the regions matching a typed phrase -- but
its viewer is not in its tree ("Support demo for arbitrary scenes" is on its TODO list; ``run/evaluate.py:343-376`` exports
coloured point clouds for an outside viewer).  And ``scripts/feature_fusion/nuscenes_openseg.py`` fuses without a depth
image (``compute_mapping(..., depth=None)``), so features bleed through walls.  One point-splat z-buffer closes both:

    Cameras       poses and pinhole intrinsics of V views (host, float64); look_at and orbit constructors
    rasterize     xyz + Cameras -> Raster: per view and pixel the nearest point (point_id) and its depth
    Raster        .colors(rgb) / .labels(labels, palette) / .heat(values, lo, hi) -> uint8 [V, H, W, 3] pictures;
                  .fusion_depth(v) -> the depth image PointCloudToImageMapper.compute_mapping(depth=...) takes
    palette(n)    a fixed colour table; default_lut() the 256-entry heat ramp
    (openscene_amd.io.save_png writes a picture; SearchResult.render shades a search's heat column in place)

A point's centre pixel is bit for bit the pixel ``compute_mapping`` gives it (one shared projection body), the nearest
float32 depth wins a pixel and equal depths go to the lower point index: a pure function of the inputs.
Kernels: csrc/render.hip through ops.render_splat / ops.render_shade; no CPU path.
"""
import colorsys
import math

import numpy as np
import torch

from . import ops
from .fusion import make_intrinsic

OTHER = (255, 0, 255)              # NaN heat, labels outside the palette
BACKGROUND = (0, 0, 0)


def palette(n):
    """uint8 [n, 3]: n distinct colours, the same on every call -- hues a golden-ratio step apart, three value levels."""
    rows = []
    for i in range(int(n)):
        h = (i * 0.6180339887498949) % 1.0
        r, g, b = colorsys.hsv_to_rgb(h, 0.55 + 0.15 * (i % 3), 1.0 - 0.2 * ((i // 3) % 3))
        rows.append((int(round(r * 255)), int(round(g * 255)), int(round(b * 255))))
    return torch.tensor(rows, dtype=torch.uint8).reshape(-1, 3)


def default_lut():
    """uint8 [256, 3]: the heat ramp -- dark blue, blue, cyan, yellow, red -- linear between five anchors."""
    anchors = np.array([(0, 0, 96), (0, 64, 255), (0, 224, 224), (255, 232, 0), (224, 0, 0)], dtype=np.float64)
    x = np.linspace(0.0, 1.0, 256)
    at = np.linspace(0.0, 1.0, len(anchors))
    lut = np.stack([np.interp(x, at, anchors[:, c]) for c in range(3)], axis=1)
    return torch.from_numpy(np.rint(lut).astype(np.uint8))


def _unit(v, what):
    norm = np.linalg.norm(v, axis=-1, keepdims=True)
    if not np.all(norm > 0):
        raise ValueError("%s has no direction" % what)
    return v / norm


class Cameras:
    """V pinhole views.  camera_to_world float64 [V, 4, 4] (x right, y down, z forward: the convention of the reference's
    pose files); intrinsic (fx, fy, cx, cy) for all views or [V, 4]; image_hw = (H, W).  Host-side float64;
    world_to_camera is np.linalg.inv of every pose, exactly as PointCloudToImageMapper computes it."""

    def __init__(self, camera_to_world, intrinsic, image_hw):
        c2w = np.array(camera_to_world, dtype=np.float64)
        if c2w.ndim == 2:
            c2w = c2w[None]
        if c2w.ndim != 3 or c2w.shape[1:] != (4, 4):
            raise ValueError("camera_to_world must be [V, 4, 4] (got %s)" % (c2w.shape,))
        k = np.array(intrinsic, dtype=np.float64)
        if k.shape == (4,):
            k = np.broadcast_to(k, (c2w.shape[0], 4)).copy()
        if k.shape != (c2w.shape[0], 4):
            raise ValueError("intrinsic must be (fx, fy, cx, cy) or [V, 4] (got %s)" % (k.shape,))
        h, w = int(image_hw[0]), int(image_hw[1])
        if h < 1 or w < 1:
            raise ValueError("image_hw must be at least 1 x 1 (got %r)" % (image_hw,))
        self.camera_to_world = c2w
        self.intrinsic = k
        self.image_hw = (h, w)
        self.world_to_camera = np.stack([np.linalg.inv(m) for m in c2w]) if len(c2w) else np.zeros((0, 4, 4))

    def __len__(self):
        return self.camera_to_world.shape[0]

    def intrinsic_matrix(self, v):
        """The 4 x 4 pinhole matrix of view v, as compute_mapping(intrinsic=...) takes it."""
        return make_intrinsic(*self.intrinsic[v])

    @classmethod
    def look_at(cls, eyes, targets, up=(0.0, 0.0, 1.0), fov_deg=60.0, image_hw=(480, 640)):
        """Cameras at `eyes` [V, 3] looking at `targets` [V, 3] (or one for all).  fov_deg is the horizontal field of view
        over the W pixels; square pixels; the principal point is the image centre ((W - 1) / 2, (H - 1) / 2), where the
        target projects."""
        eyes = np.atleast_2d(np.asarray(eyes, dtype=np.float64))
        targets = np.broadcast_to(np.atleast_2d(np.asarray(targets, dtype=np.float64)), eyes.shape)
        h, w = int(image_hw[0]), int(image_hw[1])
        if not 0.0 < float(fov_deg) < 180.0:
            raise ValueError("fov_deg must lie in (0, 180) (got %r)" % (fov_deg,))
        fwd = _unit(targets - eyes, "a camera on its target")
        right = _unit(np.cross(fwd, np.broadcast_to(np.asarray(up, dtype=np.float64), eyes.shape)), "a view along `up`")
        down = np.cross(fwd, right)
        c2w = np.zeros((eyes.shape[0], 4, 4))
        c2w[:, :3, 0], c2w[:, :3, 1], c2w[:, :3, 2], c2w[:, :3, 3] = right, down, fwd, eyes
        c2w[:, 3, 3] = 1.0
        f = 0.5 * w / math.tan(math.radians(float(fov_deg)) / 2.0)
        return cls(c2w, (f, f, 0.5 * (w - 1), 0.5 * (h - 1)), (h, w))

    @classmethod
    def orbit(cls, xyz, n_views, elevation_deg=30.0, margin=1.2, fov_deg=60.0, image_hw=(480, 640), up_axis=2):
        """n_views cameras on a circle around the bounding box of xyz [N, 3], `elevation_deg` above its centre, all looking
        at the centre from the distance at which the box's bounding sphere, grown by `margin` (>= 1), fits the narrower
        field of view: every corner of the box is inside every view."""
        n_views = int(n_views)
        if n_views < 1 or not margin >= 1.0:
            raise ValueError("orbit needs n_views >= 1 and margin >= 1")
        if isinstance(xyz, torch.Tensor):
            lo, hi = xyz.min(0)[0].double().cpu().numpy(), xyz.max(0)[0].double().cpu().numpy()
        else:
            xyz = np.asarray(xyz, dtype=np.float64)
            lo, hi = xyz.min(0), xyz.max(0)
        centre = 0.5 * (lo + hi)
        sphere = max(0.5 * float(np.linalg.norm(hi - lo)), 1e-6)
        h, w = int(image_hw[0]), int(image_hw[1])
        half_h = math.radians(float(fov_deg)) / 2.0
        half_v = math.atan(math.tan(half_h) * h / w)
        dist = float(margin) * sphere / math.sin(min(half_h, half_v))
        el = math.radians(float(elevation_deg))
        a, b = [i for i in range(3) if i != up_axis]
        eyes = np.tile(centre, (n_views, 1))
        az = 2.0 * math.pi * np.arange(n_views) / n_views
        eyes[:, a] += dist * math.cos(el) * np.cos(az)
        eyes[:, b] += dist * math.cos(el) * np.sin(az)
        eyes[:, up_axis] += dist * math.sin(el)
        up = np.zeros(3)
        up[up_axis] = 1.0
        return cls.look_at(eyes, centre, up, fov_deg, (h, w))


def _on(t, dev, name):
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a tensor" % name)
    return t.to(dev)


class Raster:
    """The z-buffer of V views of one scene: .point_id int32 [V, H, W] (-1: background), .depth float32 [V, H, W] (0:
    background), .zbuf the 64-bit keys, .n the number of points, .cameras."""

    def __init__(self, zbuf, n, cameras):
        self.zbuf = zbuf
        self.n = int(n)
        self.cameras = cameras
        self.point_id, self.depth, _ = ops.render_shade(zbuf, self.n)

    @property
    def device(self):
        return self.zbuf.device

    def colors(self, rgb, background=BACKGROUND):
        """uint8 [V, H, W, 3]: every pixel in its point's colour; rgb uint8 [n, 3]."""
        return ops.render_shade(self.zbuf, self.n, "colors", colors=_on(rgb, self.device, "rgb").contiguous(), background=background)[2]

    def labels(self, labels, palette, other=OTHER, background=BACKGROUND):
        """uint8 [V, H, W, 3]: palette[labels[point]]; labels int32 / int64 [n], palette uint8 [C, 3]; a label outside
        [0, C) (255 or -100 for "ignore", say) is drawn in `other`."""
        return ops.render_shade(self.zbuf, self.n, "labels", values=_on(labels, self.device, "labels"),
                                table=_on(palette, self.device, "palette").contiguous(), other=other, background=background)[2]

    def heat(self, values, lo, hi, lut=None, base=None, column=0, other=OTHER, background=BACKGROUND):
        """uint8 [V, H, W, 3]: values fp16 / fp32 [n], or [n, Q] with `column` (used in place), through the 256-entry `lut`
        (default_lut() when None) between lo and hi.  A point below lo is drawn in base[point] (uint8 [n, 3]: the scene in
        its own colours with the hits highlighted) or, without a base, in lut[0]; NaN in `other`."""
        lut = default_lut() if lut is None else lut
        base = None if base is None else _on(base, self.device, "base").contiguous()
        return ops.render_shade(self.zbuf, self.n, "heat", colors=base, values=_on(values, self.device, "values"), column=column,
                                table=_on(lut, self.device, "lut").contiguous(), lo=lo, hi=hi, other=other, background=background)[2]

    def fusion_depth(self, v):
        """float64 [H, W]: view v's depth image in metres as compute_mapping(depth=...) takes it (0 where nothing was drawn,
        which the occlusion test rejects)."""
        return self.depth[int(v)].double()


def rasterize(xyz, cameras, radius=0.02, max_px=4, near=0.05, device="cuda"):
    """Splat the points xyz [N, 3] (tensor or numpy; a numpy array goes to `device`) into every view of `cameras`: a point
    covers the disc of min(max_px, rint(radius * fx / depth)) pixels around its centre pixel (radius in metres; 0: one
    pixel), points nearer than `near` are not drawn.  -> Raster"""
    if not isinstance(cameras, Cameras):
        raise TypeError("cameras must be a Cameras")
    if isinstance(xyz, np.ndarray):
        xyz = torch.from_numpy(np.ascontiguousarray(xyz, dtype=np.float64)).to(device)
    if not isinstance(xyz, torch.Tensor) or xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError("xyz must be [N, 3]")
    xyz = xyz.to(torch.float64).contiguous()
    zbuf = ops.render_splat(xyz, cameras.world_to_camera, cameras.intrinsic, cameras.image_hw, radius=radius, max_px=max_px, near=near)
    return Raster(zbuf, xyz.shape[0], cameras)
