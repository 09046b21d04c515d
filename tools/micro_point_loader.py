"""Cost of Point3DLoader's per-item work on the GPU (csrc/elastic.hip, openscene_amd.loader.point_item) against the same
steps on the CPU as the reference runs them (dataset/augmentation.py:159-201 through scipy, the voxeliser through numpy).

    python tools/micro_point_loader.py [iters] [--out FILE]

Seeded ScanNet-sized rooms of 150 k and 550 k points.  Prints one JSON object per line (and appends it to FILE):
  kind=field  per (n, granularity, magnitude): device time of osn_bbox, osn_elastic_blur and osn_elastic_apply (HIP
              events around `iters` back-to-back calls), the apply pass's 48 B/point as a share of the 8 TB/s HBM roof,
              the host draw of the noise on its own, one whole ops.elastic_distort field (read-back, draw, uploads,
              kernels) in wall time, and the reference's field (numpy + scipy) on the CPU
  kind=item   per n: point_item wall time (synchronised) with and without aug (input_color=True), against the CPU's
              two distortion fields + the numpy voxeliser (floor, shift, first-occurrence quantisation of
              oracle/voxelize.py); the CPU's chromatic transforms are not counted
Threads: torch and numpy are held to 16 CPU threads; scipy's ndimage / RegularGridInterpolator are single-threaded."""
import json
import os
import random
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "16")
import numpy as np                                                      # noqa: E402
import torch                                                            # noqa: E402
from scipy import ndimage                                               # noqa: E402
from scipy.interpolate import RegularGridInterpolator                   # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openscene_amd import ops                                           # noqa: E402
from openscene_amd.loader import PointLoader, TrainAugmentation, point_item   # noqa: E402
from openscene_amd.voxelizer import Voxelizer                           # noqa: E402
from oracle import voxelize as ov                                       # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
ITERS = int(args[0]) if args else 100
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
HBM_ROOF = 8.0e12
torch.set_num_threads(16)
dev = torch.device("cuda", 0)


def emit(d):
    line = json.dumps(d)
    print(line, flush=True)
    if OUT:
        with open(OUT, "a") as f:
            f.write(line + "\n")


def timed(f, iters=ITERS, warmup=5):
    """us per call: device events around `iters` back-to-back calls."""
    for _ in range(warmup):
        f()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def wall(f, iters, warmup=2, sync=True):
    """median us per call of the host wall clock (synchronised after every call)."""
    for _ in range(warmup):
        f()
    ts = []
    for _ in range(iters):
        if sync:
            torch.cuda.synchronize()
        t = time.perf_counter()
        f()
        if sync:
            torch.cuda.synchronize()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)) * 1e6


def room(n, seed):
    rng = np.random.default_rng(seed)
    x = rng.random((n, 3)) * np.asarray((8.0, 6.0, 3.0)) - np.asarray((1.0, 2.0, 0.0))
    x[: n // 4, 2] = rng.normal(0, 0.01, n // 4)
    x[n // 4: 2 * (n // 4), 0] = np.where(rng.random(n // 4) < 0.5, -1.0, 7.0) + rng.normal(0, 0.01, n // 4)
    return x


def cpu_blur(noise):
    bx = np.ones((3, 1, 1, 1)).astype("float32") / 3
    by = np.ones((1, 3, 1, 1)).astype("float32") / 3
    bz = np.ones((1, 1, 3, 1)).astype("float32") / 3
    for _ in range(2):
        noise = ndimage.convolve(noise, bx, mode="constant", cval=0)
        noise = ndimage.convolve(noise, by, mode="constant", cval=0)
        noise = ndimage.convolve(noise, bz, mode="constant", cval=0)
    return noise


def cpu_field(coords, granularity, magnitude):
    """ElasticDistortion.elastic_distortion as the reference calls numpy / scipy."""
    coords_min = coords.min(0)
    noise_dim = ((coords - coords_min).max(0) // granularity).astype(int) + 3
    noise = cpu_blur(np.random.randn(*noise_dim, 3).astype(np.float32))
    ax = [np.linspace(d_min, d_max, d) for d_min, d_max, d in
          zip(coords_min - granularity, coords_min + granularity * (noise_dim - 2), noise_dim)]
    return coords + RegularGridInterpolator(ax, noise, bounds_error=0, fill_value=0)(coords) * magnitude


def cpu_voxelize(xyz, vox):
    M_v, M_r = vox.get_transformation_matrix()
    return ov.voxelize_with_matrix(xyz, M_r @ M_v)


def main():
    params = PointLoader.ELASTIC_DISTORT_PARAMS
    for n in (150000, 550000):
        x_np = room(n, seed=n)
        x = torch.from_numpy(x_np).to(dev)
        for g, m in params:
            box = ops.bbox(x)
            lo, hi = box.cpu().numpy()[:3], box.cpu().numpy()[3:]
            nd = ((hi - lo) // g).astype(int) + 3
            ax = [np.linspace(a, b, k) for a, b, k in zip(lo - g, lo + g * (nd - 2), nd)]
            noise = torch.from_numpy(np.random.default_rng(0).standard_normal((*nd, 3)).astype(np.float32)).to(dev)
            t_bbox = timed(lambda: ops.bbox(x))
            t_blur = timed(lambda: ops.elastic_blur(noise))
            t_apply = timed(lambda: ops.elastic_apply(x, noise, ax, m))
            t_draw = wall(lambda: np.random.randn(*nd, 3).astype(np.float32), 20, sync=False)
            t_field = wall(lambda: ops.elastic_distort(x, g, m, bbox6=box), 20)
            t_cpu = wall(lambda: cpu_field(x_np, g, m), 3, warmup=1, sync=False)
            bytes_apply = 48 * n
            emit(dict(kind="field", n=n, granularity=g, magnitude=m, grid=[int(v) for v in nd],
                      us_bbox=round(t_bbox, 2), us_blur=round(t_blur, 2), us_apply=round(t_apply, 2),
                      apply_bytes=bytes_apply, apply_hbm_roof_us=round(bytes_apply / HBM_ROOF * 1e6, 2),
                      apply_share_of_roof=round(bytes_apply / HBM_ROOF * 1e6 / t_apply, 3),
                      us_host_noise_draw=round(t_draw, 1), us_field_wall=round(t_field, 1), us_cpu_field=round(t_cpu, 1)))
        # one whole item, both ways
        rng = np.random.default_rng(n + 1)
        colors = torch.from_numpy(rng.random((n, 3)) * 255).to(dev)
        labels = torch.from_numpy(rng.integers(0, 20, n).astype(np.uint8)).to(dev)
        vox = Voxelizer(voxel_size=0.02, clip_bound=None, use_augmentation=True,
                        scale_augmentation_bound=PointLoader.SCALE_AUGMENTATION_BOUND,
                        rotation_augmentation_bound=PointLoader.ROTATION_AUGMENTATION_BOUND,
                        translation_augmentation_ratio_bound=PointLoader.TRANSLATION_AUGMENTATION_RATIO_BOUND, device=dev)
        aug = TrainAugmentation(params)
        np.random.seed(1)
        random.seed(1)
        t_item_aug = wall(lambda: point_item(vox, x, colors, labels, input_color=True, aug=aug), 20)
        t_item = wall(lambda: point_item(vox, x, colors, labels, input_color=True), 20)

        def cpu_item():
            y = x_np
            for g, m in params:
                y = cpu_field(y, g, m)
            return cpu_voxelize(y, vox)
        t_cpu_item = wall(cpu_item, 3, warmup=1, sync=False)
        t_cpu_vox = wall(lambda: cpu_voxelize(x_np, vox), 3, warmup=1, sync=False)
        emit(dict(kind="item", n=n, voxel_size=0.02, us_point_item_aug=round(t_item_aug, 1),
                  us_point_item_no_aug=round(t_item, 1), us_cpu_distort_and_voxelize=round(t_cpu_item, 1),
                  us_cpu_voxelize_only=round(t_cpu_vox, 1)))


if __name__ == "__main__":
    main()
