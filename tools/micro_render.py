"""Cost of rendering scene views (csrc/render.hip) against the same result written with what torch offers, measured in the
same process:

  splat        ops.render_splat: the z-buffers of all views (one memset, one launch per view)
  shade        ops.render_shade in the heat mode with a base image (point ids, depths and the picture, one launch)
  torch splat  per view: the projection in float64 (matmul, multiply, divide, add, round), int64 keys, the footprints
               expanded to [n, K] pixel candidates (K = the offsets of a disc of max_px; 1 when radius == 0), a boolean
               mask, and ONE scatter_reduce(amin) per view
  torch shade  the ids and depths by shifts and masks, gathers of the heat column, the LUT and the base, torch.where

    python tools/micro_render.py [iters] [out.jsonl]

One 150 k-point scene (openscene_amd.synthetic room), 8 orbit views at 640 x 480, radius 0 and 0.02 m (max_px 4).  HIP
events around windows of about a quarter of a second of back-to-back calls after a warm-up; the variants alternate and the
median of three rounds is reported (rounds_us keeps all of them).  The z-buffers (8 x 640 x 480 x 8 bytes = 19.7 MB) and the
points (3.6 MB) stay in the last-level cache between the calls of a window, for both routes.  The two routes are compared
pixel by pixel; torch's float64 matmul is not the kernel's FMA chain, so a handful of half-pixel ties may differ (counted).
`atomics` counts the candidates (point, pixel) pairs of the footprints: the atomics an unfiltered kernel would issue.
One JSON object per line (also appended to out.jsonl when given)."""
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openscene_amd import ops                                        # noqa: E402
from openscene_amd import render as R                                # noqa: E402
from openscene_amd import synthetic as syn                           # noqa: E402

ITERS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
OUT = sys.argv[2] if len(sys.argv) > 2 else None
dev = torch.device("cuda", 0)
ROUNDS = 3
WINDOW_US = 250_000.0
N, VIEWS, HW = 150_000, 8, (480, 640)
MAX_PX, NEAR = 4, 0.05
LO, HI = 0.5, 1.0
FAR = torch.iinfo(torch.int64).max


def events_us(f, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def rounds(fs):
    """us per call of every function of `fs`: a warm-up, then ROUNDS alternating rounds, each timing a window of about
    WINDOW_US (at most ITERS * 50 calls) between device events; (medians, all rounds, calls per window)."""
    iters = []
    for f in fs:
        f()
        f()
        torch.cuda.synchronize()
        est = events_us(f, 3)
        iters.append(max(3, min(ITERS * 50, int(WINDOW_US / max(est, 1.0)))))
    got = [[] for _ in fs]
    for _ in range(ROUNDS):
        for i, f in enumerate(fs):
            got[i].append(events_us(f, iters[i]))
    return [statistics.median(g) for g in got], got, iters


def emit(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    if OUT:
        with open(OUT, "a") as fh:
            fh.write(line + "\n")


def disc(max_px):
    return [(dx, dy) for dy in range(-max_px, max_px + 1) for dx in range(-max_px, max_px + 1) if dx * dx + dy * dy <= max_px * max_px]


def torch_splat(xyz1, w2c, k4, radius, stats=None):
    """int64 [V, H, W] keys (FAR: background) with torch.  xyz1 float64 [4, n] (the points with a row of ones), w2c float64
    [V, 4, 4] on the device, k4 the host intrinsics."""
    h, w = HW
    n = xyz1.shape[1]
    index = torch.arange(n, device=dev)
    offs = torch.tensor(disc(MAX_PX) if radius > 0 else [(0, 0)], device=dev)
    dx, dy = offs[:, 0][None, :], offs[:, 1][None, :]
    d2 = dx * dx + dy * dy
    z = torch.full((w2c.shape[0], h * w), FAR, dtype=torch.int64, device=dev)
    for v in range(w2c.shape[0]):
        fx, fy, cx, cy = (float(x) for x in k4[v])
        p = w2c[v] @ xyz1
        p2 = p[2]
        u = torch.round((p[0] * fx) / p2 + cx)
        r_ = torch.round((p[1] * fy) / p2 + cy)
        zf = p2.float()
        ok = (p2 >= NEAR) & ~torch.isinf(zf) & (u.abs() < 2.0 ** 30) & (r_.abs() < 2.0 ** 30)
        rad = torch.round((radius * fx) / p2).clamp(0, MAX_PX).nan_to_num(0.0).long() if radius > 0 else torch.zeros_like(index)
        key = (zf.view(torch.int32).long() << 32) | index
        cu, cv = u.nan_to_num(0.0).clamp(-2.0 ** 30, 2.0 ** 30).long(), r_.nan_to_num(0.0).clamp(-2.0 ** 30, 2.0 ** 30).long()
        x, y = cu[:, None] + dx, cv[:, None] + dy
        m = ok[:, None] & (d2 <= (rad * rad)[:, None]) & (x >= 0) & (x < w) & (y >= 0) & (y < h)
        z[v].scatter_reduce_(0, (y * w + x)[m], key[:, None].expand(-1, offs.shape[0])[m], "amin")
        if stats is not None:
            stats["atomics"] = stats.get("atomics", 0) + int(m.sum())
    return z.view(-1, h, w)


def torch_shade(z, heat_col, lut, base, other, background):
    bg = z == FAR
    pid = torch.where(bg, torch.full_like(z, -1), z & 0xFFFFFFFF).int()
    depth = torch.where(bg, torch.zeros_like(z), z >> 32).int().view(torch.float32)
    i = pid.long().clamp(min=0)
    hval = heat_col[i].float()
    t = (hval - LO) / (HI - LO)
    rgb = lut[torch.round(t * 255.0).nan_to_num(0.0).clamp(0, 255).long()]
    rgb = torch.where((hval < LO)[..., None], base[i], rgb)
    rgb = torch.where(torch.isnan(hval)[..., None], other, rgb)
    rgb = torch.where(bg[..., None], background, rgb)
    return pid, depth, rgb


def case(radius, gen):
    xyz_host = syn.room_points(0, n_pts=N)
    xyz = torch.from_numpy(np.ascontiguousarray(xyz_host, dtype=np.float64)).to(dev)
    n = xyz.shape[0]
    cams = R.Cameras.orbit(xyz, VIEWS, image_hw=HW)
    rgb = torch.randint(0, 256, (n, 3), generator=gen, device=dev, dtype=torch.uint8)
    heat = torch.rand((n, 5), generator=gen, device=dev).half()
    lut = R.default_lut().to(dev)
    other = torch.tensor(R.OTHER, dtype=torch.uint8, device=dev)
    background = torch.tensor(R.BACKGROUND, dtype=torch.uint8, device=dev)
    xyz1 = torch.cat([xyz, torch.ones((n, 1), dtype=torch.float64, device=dev)], 1).t().contiguous()
    w2c = torch.from_numpy(cams.world_to_camera).to(dev)
    k4 = cams.intrinsic

    def ours_splat():
        return ops.render_splat(xyz, cams.world_to_camera, k4, HW, radius=radius, max_px=MAX_PX, near=NEAR)

    def ours_shade(z):
        return ops.render_shade(z, n, "heat", colors=rgb, values=heat, column=3, table=lut, lo=LO, hi=HI)

    z = ours_splat()
    stats = {}
    zt = torch_splat(xyz1, w2c, k4, radius, stats)
    heat_col = heat[:, 3]
    a, b = ours_shade(z), torch_shade(zt, heat_col, lut, rgb, other, background)
    total = z.numel()
    differ = int((a[0] != b[0]).sum())
    assert differ <= total // 1000, differ                                   # (half-pixel ties of the two matmuls only)
    same = a[0] == b[0]
    assert torch.equal(a[1][same].view(torch.int32), b[1][same].view(torch.int32)) and torch.equal(a[2][same], b[2][same])
    (us_splat, us_shade, us_torch_splat, us_torch_shade), spread, iters = rounds([
        ours_splat, lambda: ours_shade(z), lambda: torch_splat(xyz1, w2c, k4, radius), lambda: torch_shade(zt, heat_col, lut, rgb, other, background)])
    drawn = int((a[0] >= 0).sum())
    emit(kind="render", points=n, views=VIEWS, image_hw=list(HW), radius=radius, max_px=MAX_PX, near=NEAR, pixels=total, pixels_drawn=drawn,
         atomics=stats["atomics"], pixels_differing_between_routes=differ, us_splat=us_splat, us_shade=us_shade,
         us_torch_splat=us_torch_splat, us_torch_shade=us_torch_shade, torch_over_splat=us_torch_splat / us_splat,
         torch_over_shade=us_torch_shade / us_shade, splat_candidates_per_us=stats["atomics"] / us_splat,
         shade_bytes=total * (8 + 4 + 4 + 3), shade_bytes_per_s=total * (8 + 4 + 4 + 3) / (us_shade * 1e-6),
         rounds_us=spread, calls_per_window=iters, window_us=WINDOW_US)


if __name__ == "__main__":
    g = torch.Generator(device=dev).manual_seed(1)
    np.random.seed(0)
    for radius in (0.0, 0.02):
        case(radius, g)
