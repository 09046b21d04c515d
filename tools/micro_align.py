"""Cost of aligning two scans (csrc/align.hip, openscene_amd.align) against the same quantities composed in torch on the same
device: the residuals of a chunk of hypotheses as an ``einsum`` into a [chunk, P, 3] temporary (held to 1 GiB), a comparison
and a sum over P.  HIP events around back-to-back calls after a warm-up, in windows of at least 50 ms; the drivers, which
synchronise, are timed with a host clock around calls that end in a synchronise.

    python tools/micro_align.py [iters] [--out FILE]

Prints (and with --out also writes) one JSON object per line:
  kind=align_score     H = 4096 hypotheses x P in {1 k, 20 k, 100 k} pairs of a planted problem (40 % outliers)
    case                 4096_x_P: the hypotheses the congruence pre-test left valid are scored (`scored` of them), as
                         estimate_rigid does; 4096_x_P_all_scored: valid = None, all H x P residuals
    us                   one ops.rigid_score call as a user makes it: two launches, one allocation, the Python around them
    us_kernels           the C entry alone on a preallocated `counts`
    residuals            H x P; valu_ops = 22 per residual (9 multiplies, 9 additions, 3 subtractions, a compare: the contract
                         forbids FMA); valu_share = valu_ops / us_kernels over 256 CUs x 128 lanes x 2.4 GHz
    us_torch             the torch route in chunks of `torch_chunk` hypotheses; torch_temp_bytes = one chunk's temporaries.
                         Not of equal rounding (einsum fuses and reorders): counts_agree is the share of hypotheses on which
                         the two routes count the same, not a parity check
  kind=align_triplets  ops.rigid_from_triplets of H = 4096
  kind=align_moments   ops.rigid_moments at the planted transform (P as above), beside float64 masked sums in torch
  kind=align_estimate  the whole estimate_rigid (H = 4096, refine = 3): host clock, ends in a synchronise; `count` of `planted`
  kind=align_icp       one ICP round at 150 k points of synthetic.room_points on a 5 cm grid: the search (PointIndex.knn),
                       us_knn, the moments from the neighbour list us_moments, and us_round = refine_icp(iterations=0): one search,
                       one moments call and the synchronising read of the 16 sums (host clock); us_torch_moments = the torch route
                       given the same neighbour list (a gathered copy of B, float64 masked sums); us_refine_icp = the whole loop
                       from a 0.3 degree, 7 mm offset (`iterations` Kabsch steps, each a 3 x 3 SVD on the host)"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openscene_amd import _lib, align, ops                           # noqa: E402
from openscene_amd.ops import _p, _stream                            # noqa: E402

ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
OUT = None
if "--out" in sys.argv:
    OUT = sys.argv[sys.argv.index("--out") + 1]
    ARGS = [a for a in ARGS if a != OUT]
ITERS = int(ARGS[0]) if ARGS else 3
WINDOW_MS = 50.0
dev = torch.device("cuda", 0)
VALU_PEAK = 256 * 128 * 2.4e9                                        # float32 lane-operations per second
VALU_PER_RESIDUAL = 22
H = 4096
THRESHOLD = 0.01
TEMP_BYTES = 1 << 30
_lines = []


def timed(f, iters=ITERS, warmup=1, window_ms=WINDOW_MS):
    """(us per call, calls): device events around back-to-back calls, at least `iters` of them and at least `window_ms` long."""
    for _ in range(warmup):
        f()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    while True:
        a.record()
        for _ in range(iters):
            f()
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b)
        if ms >= window_ms:
            return ms * 1e3 / iters, iters
        iters = int(iters * 1.2 * window_ms / max(ms, 1e-3)) + 1


def host_timed(f, iters=ITERS, warmup=1, window_s=0.2):
    """(us per call, calls) by the host clock; f synchronises before it returns."""
    for _ in range(warmup):
        f()
    while True:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            f()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dt >= window_s:
            return dt * 1e6 / iters, iters
        iters = int(iters * 1.2 * window_s / max(dt, 1e-6)) + 1


def emit(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    _lines.append(line)


def rotation(axis, degrees):
    k = np.asarray(axis, dtype=np.float64)
    k = k / np.linalg.norm(k)
    a = np.deg2rad(degrees)
    kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(a) * kx + (1 - np.cos(a)) * (kx @ kx)


BOX = np.array([4.8, 3.6, 2.4])
TRUTH = align.RigidTransform(rotation((0.3, -0.5, 0.81), 37.0), [0.7, -1.3, 0.25])


def planted(p, seed=0, outliers=0.4, noise=0.002):
    rng = np.random.default_rng(seed)
    src = rng.random((p, 3)) * BOX
    dst = TRUTH.apply(src) + rng.uniform(-noise, noise, (p, 3))
    out = rng.permutation(p)[:int(round(outliers * p))]
    dst[out] = TRUTH.apply(rng.random((out.shape[0], 3)) * BOX)
    return torch.from_numpy(src.astype(np.float32)).to(dev), torch.from_numpy(dst.astype(np.float32)).to(dev), p - out.shape[0]


def torch_score(src, dst, xf, valid, tau2, chunk):
    counts = torch.empty(xf.shape[0], dtype=torch.int32, device=dev)
    for h0 in range(0, xf.shape[0], chunk):
        x = xf[h0:h0 + chunk]
        e = torch.einsum("hij,pj->hpi", x[:, :9].reshape(-1, 3, 3), src) + x[:, None, 9:] - dst[None]
        counts[h0:h0 + chunk] = ((e * e).sum(-1) <= tau2).sum(1)
    return torch.where(valid, counts, torch.full_like(counts, -1))


def torch_moments(src, dst, xf12, tau2, idx=None):
    x = torch.from_numpy(np.asarray(xf12, dtype=np.float32)).to(dev)
    if idx is not None:
        has = (idx >= 0) & (idx < dst.shape[0])
        dst = dst[idx.clamp(0, dst.shape[0] - 1).long()]            # the gathered copy
    e = src @ x[:9].reshape(3, 3).T + x[9:] - dst
    r2 = (e * e).sum(-1)
    inl = r2 <= tau2
    if idx is not None:
        inl = inl & has
        r2 = torch.where(has, r2, torch.full_like(r2, float("inf")))
    s, d = src.double() * inl[:, None], dst.double() * inl[:, None]
    return inl, r2, torch.cat([inl.sum()[None].double(), s.sum(0), d.sum(0), (s.T @ d).reshape(9)])


def score_cases():
    lib = _lib.load()
    tau2 = align._tau2(THRESHOLD)
    for name, p in (("1k", 1000), ("20k", 20000), ("100k", 100000)):
        src, dst, n_in = planted(p)
        trip = align.draw_triplets(p, H, 0).to(dev)
        area2 = align.area2_min_of(THRESHOLD)
        xf, valid = ops.rigid_from_triplets(src, dst, trip, THRESHOLD, area2)
        us_trip, _ = timed(lambda: ops.rigid_from_triplets(src, dst, trip, THRESHOLD, area2))
        emit(kind="align_triplets", pairs=p, hypotheses=H, us=us_trip, valid=int(valid.sum()))
        got = ops.rigid_score(src, dst, xf, tau2, valid)
        chunk = max(1, min(H, TEMP_BYTES // (p * 12 * 3)))            # e, e * e and the einsum's own output
        want = torch_score(src, dst, xf, valid, tau2, chunk)
        agree = float((got == want).double().mean())
        counts = torch.empty(H, dtype=torch.int32, device=dev)
        st = _stream(dev)

        def raw(mask):
            rc = lib.osn_rigid_score(_p(src), _p(dst), p, _p(xf), _p(mask), H, tau2, _p(counts), st)
            if rc != 0:
                raise SystemExit("osn_rigid_score returned %d" % rc)
        us_torch, _ = timed(lambda: torch_score(src, dst, xf, valid, tau2, chunk), iters=1)
        for case, mask in (("4096_x_" + name, valid), ("4096_x_" + name + "_all_scored", None)):       # (None: every one of the H is scored)
            us, calls = min(timed(lambda: ops.rigid_score(src, dst, xf, tau2, mask)) for _ in range(2))
            us_kernels, _ = min(timed(lambda: raw(mask)) for _ in range(2))
            scored = H if mask is None else int(mask.sum())
            emit(kind="align_score", case=case, pairs=p, hypotheses=H, scored=scored, us=us, calls=calls, us_kernels=us_kernels,
                 us_torch=us_torch, speedup=us_torch / us, residuals=scored * p, valu_ops=VALU_PER_RESIDUAL * scored * p,
                 valu_share=VALU_PER_RESIDUAL * scored * p / us_kernels * 1e6 / VALU_PEAK, torch_chunk=chunk,
                 torch_temp_bytes=chunk * p * 12 * 3, counts_agree=agree, best=int(got.max()), planted=n_in)
        x12 = TRUTH.float32()
        us_m, _ = min(timed(lambda: ops.rigid_moments(src, dst, x12, tau2)) for _ in range(2))
        us_mt, _ = timed(lambda: torch_moments(src, dst, x12, tau2))
        m = ops.rigid_moments(src, dst, x12, tau2)[2]
        gap = float((m - torch_moments(src, dst, x12, tau2)[2]).abs().max())
        emit(kind="align_moments", pairs=p, us=us_m, us_torch=us_mt, speedup=us_mt / us_m, inliers=int(m[0]), max_abs_gap_to_torch=gap)
        fit = align.estimate_rigid(src, dst, THRESHOLD, hypotheses=H, seed=0)
        us_e, calls_e = host_timed(lambda: align.estimate_rigid(src, dst, THRESHOLD, hypotheses=H, seed=0))
        emit(kind="align_estimate", pairs=p, hypotheses=H, refine=3, us=us_e, calls=calls_e, count=fit.count, planted=n_in, ok=fit.ok)


def icp_case(n=150_000):
    from openscene_amd.neighbors import PointIndex
    from openscene_amd.objects import VoxelGrid
    from openscene_amd.synthetic import room_points
    b = room_points(0, n_pts=n).astype(np.float32)
    move = align.RigidTransform(rotation((0.2, 0.1, 1.0), 0.3), [0.006, -0.004, 0.002])
    a = torch.from_numpy(move.apply(b).astype(np.float32)).to(dev)
    index = PointIndex(VoxelGrid(torch.from_numpy(b).to(dev), voxel_size=0.05))
    tau2 = align._tau2(0.05)
    eye = align.RigidTransform()
    x12 = eye.float32()
    us_knn, _ = timed(lambda: index.knn(eye.apply(a), 1, radius=0.05))
    idx = index.knn(eye.apply(a), 1, radius=0.05).idx[:, 0].contiguous()
    us_m, _ = min(timed(lambda: ops.rigid_moments(a, index.grid.xyz, x12, tau2, dst_idx=idx)) for _ in range(2))
    us_mt, _ = timed(lambda: torch_moments(a, index.grid.xyz, x12, tau2, idx))
    us_round, calls = host_timed(lambda: align.refine_icp(index, a, eye, iterations=0, radius=0.05))
    fit = align.refine_icp(index, a, eye, iterations=10, radius=0.05)
    us_full, _ = host_timed(lambda: align.refine_icp(index, a, eye, iterations=10, radius=0.05), iters=1)
    twins = float((fit.neighbors.cpu() == torch.arange(n, dtype=torch.int32)).double().mean())
    emit(kind="align_icp", points=n, voxel_size=0.05, us_knn=us_knn, us_moments=us_m, us_torch_moments=us_mt, us_round=us_round, calls=calls,
         paired=int((idx >= 0).sum()), us_refine_icp=us_full, iterations=fit.iterations, count=fit.count, twins=twins)


def main():
    score_cases()
    icp_case()
    if OUT:
        os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
        with open(OUT, "w") as f:
            f.write("\n".join(_lines) + "\n")


if __name__ == "__main__":
    main()
