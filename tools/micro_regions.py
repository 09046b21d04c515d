"""Cost of segmenting scenes without a prompt (csrc/regions.hip) against the same steps written with what torch offers,
measured in the same process:

  rows       regions.voxel_rows: one unit feature row per voxel through the pool kernel, in slices
  edges      ops.regions_edges alone, with its bytes -- V * d * 2 * (1 + present earlier neighbours per voxel) read plus the
             sim array written -- as a fraction of the HBM roof (8 TB/s): the rows are re-read once per present neighbour, and
             only as far as the order of VoxelGrid.coords is spatially coherent do the re-reads hit the L2 of their XCD
  segment    graph.segment at three thresholds (label + number + records; the dot products are not redone)
  torch      the edges as a gather of the neighbour rows and (a * b).sum(-1) per offset, and the labelling as the
             scatter_reduce(amin) label propagation of tools/micro_objects.py's torch route (one read-back per sweep)

    python tools/micro_regions.py [iters] [out.jsonl]

8 scenes x 150 k points x 768 features (openscene_amd.synthetic rooms, 5 cm voxels), both bank kinds.  The features are planted
clusters: a point takes the prototype of the nearest of 24 centres of its scene plus Gaussian noise.  HIP events around
windows of about a quarter of a second of back-to-back calls after a warm-up; the variants alternate and the median of
three rounds is reported (rounds_us keeps all of them, so the run-to-run spread stands next to every ratio).  Working sets
under 256 MB are re-read from the last-level cache between calls of a window: the rows here are larger than that, the sim
array and the label words are not.  One JSON object per line (also appended to out.jsonl when given)."""
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openscene_amd import ops                                        # noqa: E402
from openscene_amd import regions as R                               # noqa: E402
from openscene_amd import synthetic as syn                           # noqa: E402
from openscene_amd.objects import VoxelGrid                          # noqa: E402
from openscene_amd.search import FeatureBank                         # noqa: E402

ITERS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
OUT = sys.argv[2] if len(sys.argv) > 2 else None
dev = torch.device("cuda", 0)
VS = 0.05
D = 768
ROUNDS = 3
WINDOW_US = 250_000.0
HBM_ROOF = 8.0e12                # bytes per second
THRESHOLDS = (0.5, 0.8, 0.95)
BIG = 1 << 62


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
    WINDOW_US (at most ITERS * 50 calls) between device events; (medians, all rounds)."""
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


def planted_features(xyz, offsets, gen):
    """fp16 [N, D]: the prototype of the nearest of 24 centres of the point's scene, plus noise."""
    feats = torch.empty((xyz.shape[0], D), dtype=torch.float16, device=dev)
    for a, b in zip(offsets[:-1], offsets[1:]):
        pts = xyz[a:b]
        centres = pts[torch.randint(0, b - a, (24,), generator=gen, device=dev)]
        protos = torch.nn.functional.normalize(torch.randn(24, D, generator=gen, device=dev), dim=1)
        near = torch.cdist(pts, centres).argmin(1)
        for c0 in range(0, b - a, 50_000):                                   # (bounded float32 temporaries)
            c1 = min(c0 + 50_000, b - a)
            f = protos[near[c0:c1]] + 0.015 * torch.randn(c1 - c0, D, generator=gen, device=dev)
            feats[a + c0:a + c1] = f.half()
    return feats


def torch_edges(vox, nbr, ks):
    """sim [n_off, V] with torch: gather the neighbour rows, multiply, add (one offset at a time: [V, D] float32 temporaries)."""
    a = vox.float()
    out = torch.empty((len(ks), vox.shape[0]), dtype=torch.float32, device=dev)
    for i, k in enumerate(ks):
        u = nbr[k].long()
        s = (a * a[u.clamp(min=0)]).sum(-1)
        out[i] = torch.where(u >= 0, s, torch.full_like(s, float("-inf")))
    return out


def torch_label(sim, nbr, ks, thr, stats):
    """voxel_root by label propagation over the accepted edges in both directions until a fixed point."""
    v_n = sim.shape[1]
    label = torch.arange(v_n, device=dev)
    ok = sim >= thr
    src = torch.arange(v_n, device=dev)
    pairs = [(src[ok[i]], nbr[k].long()[ok[i]]) for i, k in enumerate(ks)]
    sweeps = 0
    while True:
        new = label.clone()
        for v, u in pairs:
            new.scatter_reduce_(0, v, label[u], "amin")
            new.scatter_reduce_(0, u, label[v], "amin")
        sweeps += 1
        if torch.equal(new, label):                                          # (one read-back per sweep)
            break
        label = new
    stats["sweeps"] = sweeps
    return label


def case(scenes, n, gen):
    rooms = [torch.from_numpy(syn.room_points(s, n_pts=n)) + torch.tensor([6.0 * s, 0.0, 0.0], dtype=torch.float64) for s in range(scenes)]
    xyz = torch.cat(rooms, 0).to(dev)
    offsets = [i * n for i in range(scenes + 1)]
    grid = VoxelGrid(xyz, offsets, voxel_size=VS)
    feats = planted_features(grid.xyz, offsets, gen)
    ks = list(range(13))
    v_n = grid.n_voxels
    present = int((grid.nbr[:13] >= 0).sum())
    for dtype in ("fp16", "fp8"):
        bank = FeatureBank(D, dev, capacity_rows=scenes * n, dtype=dtype)
        for s in range(scenes):
            bank.add_scene("s%d" % s, feats[offsets[s]:offsets[s + 1]])
        graph = R.SimilarityGraph(bank, grid)
        vox = graph.vox
        bytes_edges = v_n * D * 2 + present * D * 2 + 13 * v_n * 4
        (us_rows, us_edges, us_torch_edges), spread, iters = rounds([
            lambda: R.voxel_rows(bank, grid), lambda: ops.regions_edges(vox, grid.nbr, 26), lambda: torch_edges(vox, grid.nbr, ks)])
        ref = torch_edges(vox, grid.nbr, ks)
        fin = torch.isfinite(ref)
        assert torch.equal(fin, torch.isfinite(graph.sim)) and float((ref[fin] - graph.sim[fin]).abs().max()) < 1e-4
        emit(kind="edges", bank=dtype, scenes=scenes, rows_per_scene=n, d=D, voxels=v_n, voxel_size=VS,
             present_earlier_neighbours_per_voxel=present / v_n, rows_bytes=v_n * D * 2, bytes=bytes_edges, us_rows=us_rows,
             us_edges=us_edges, edges_bytes_per_s=bytes_edges / (us_edges * 1e-6), edges_fraction_of_hbm_roof=bytes_edges / (us_edges * 1e-6) / HBM_ROOF,
             edges_unique_bytes_fraction_of_hbm_roof=(v_n * D * 2 + 13 * v_n * 4) / (us_edges * 1e-6) / HBM_ROOF,
             us_torch_edges=us_torch_edges, torch_over_edges=us_torch_edges / us_edges, rounds_us=spread, calls_per_window=iters,
             window_us=WINDOW_US, hbm_roof_bytes_per_s=HBM_ROOF)
        for thr in THRESHOLDS:
            res = graph.segment(thr)
            (us_segment, us_label), spread, iters = rounds([lambda: graph.segment(thr),
                                                            lambda: ops.regions_label(graph.sim, grid.nbr, 26, thr)])
            stats = {}
            torch_label(graph.sim, grid.nbr, ks, thr, {})                      # warm-up
            us_first = events_us(lambda: torch_label(graph.sim, grid.nbr, ks, thr, stats), 1)
            calls = max(1, min(10, int(2e6 / us_first)))
            us_torch = events_us(lambda: torch_label(graph.sim, grid.nbr, ks, thr, stats), calls) if calls > 1 else us_first
            lab = torch_label(graph.sim, grid.nbr, ks, thr, stats)
            assert int((lab == torch.arange(v_n, device=dev)).sum()) == res.n_regions            # the same components
            emit(kind="segment", bank=dtype, scenes=scenes, rows_per_scene=n, voxels=v_n, similarity=thr, regions=res.n_regions,
                 largest_points=int(res.n_points.max()), us_segment=us_segment, us_label=us_label, us_torch_label=us_torch,
                 torch_calls=calls, torch_sweeps=stats["sweeps"], torch_label_over_label=us_torch / us_label, rounds_us=spread,
                 calls_per_window=iters, window_us=WINDOW_US)
        del bank, graph, vox


if __name__ == "__main__":
    g = torch.Generator(device=dev).manual_seed(1)
    np.random.seed(0)
    case(8, 150_000, g)
