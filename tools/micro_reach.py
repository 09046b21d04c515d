"""Cost of the distance-field kernel (csrc/reach.hip) against the same result written with what torch offers, measured in the
same process:

  field         openscene_amd.reach.distance_field over every voxel of the grid, from a random share of the POINTS as sources:
                  0.1 % and 2 % at reach 20        "how far is each voxel from the nearest hit"
                  70 % at reach 8                  the fill_missing shape: most voxels are sources, the rest look for one
                  2 % at reach 4096                culling by reach is moot: only the running bound prunes
                the kernel alone over a ready plan (`us_kernel`: ops.reach_run), the plan alone (`us_plan`: the two sorts by
                (scene, 8^3 block), the block table and the work items, in torch) and the whole call as a user makes it
                (`us_call`: the source mask to voxels, the plan, the kernel, the read of the error word)
  torch route   per scene, in chunks of CHUNK query cells: torch.cdist over the cells (float32: exact below 2^24), the square
                rounded back to an integer, the reach cut, the key d2 << 32 | id, a min: N x S distances per scene

    python tools/micro_reach.py [iters] [out.jsonl]

8 scenes x 150 k points (openscene_amd.synthetic rooms), 5 cm voxels.  Ours: HIP events around windows of about a quarter of a
second of back-to-back calls after a warm-up, the median of three rounds (rounds_us keeps all of them).  The torch route: one
warm-up on the first chunk of the first scene, then TORCH_PASSES whole passes, each timed between events.  `blocks_staged` and
`entries_scanned` are not measured: the kernel keeps no counters.  The two routes are compared: voxels whose (dist2, nearest)
differ are counted (none are expected: both are exact).  One JSON object per line (also appended to out.jsonl when given)."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                                                   # noqa: E402
from openscene_amd import ops                                        # noqa: E402
from openscene_amd import reach as R                                 # noqa: E402
from openscene_amd import synthetic as syn                           # noqa: E402
from openscene_amd.objects import VoxelGrid                          # noqa: E402

ITERS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
OUT = sys.argv[2] if len(sys.argv) > 2 else None
dev = torch.device("cuda", 0)
ROUNDS = 3
WINDOW_US = 250_000.0
SCENES, POINTS, VOXEL = 8, 150_000, 0.05
CHUNK = 2048
TORCH_PASSES = 2
CASES = ((0.001, 20), (0.02, 20), (0.7, 8), (0.02, 4096))


def events_us(f, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def rounds(f):
    """us per call: a warm-up, then ROUNDS windows of about WINDOW_US (at most ITERS * 50 calls) between device events;
    (median, all rounds, calls per window)."""
    f()
    f()
    torch.cuda.synchronize()
    iters = max(3, min(ITERS * 50, int(WINDOW_US / max(events_us(f, 3), 1.0))))
    got = [events_us(f, iters) for _ in range(ROUNDS)]
    return statistics.median(got), got, iters


def emit(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    if OUT:
        with open(OUT, "a") as fh:
            fh.write(line + "\n")


def torch_field(coords, held, reach, scenes=None, first_chunk_only=False):
    """(dist2 int64 [V], nearest int64 [V]) by cdist + min per scene and chunk; -1 without a source within reach."""
    v = coords.shape[0]
    dist2 = torch.full((v,), -1, dtype=torch.int64, device=dev)
    nearest = torch.full((v,), -1, dtype=torch.int64, device=dev)
    none = torch.iinfo(torch.int64).max
    rows = torch.arange(v, device=dev)
    for s in (range(SCENES) if scenes is None else scenes):
        mine = rows[coords[:, 0] == s]
        src = mine[held[mine]]
        if src.numel() == 0:
            continue
        src_xyz = coords[src, 1:].float()
        for a in range(0, mine.numel(), CHUNK):
            q = mine[a:a + CHUNK]
            d = torch.cdist(coords[q, 1:].float(), src_xyz)
            d2 = torch.round(d * d).long()
            key = torch.where(d2 <= reach * reach, (d2 << 32) | src[None, :], torch.full_like(d2, none)).min(1)[0]
            some = key != none
            dist2[q] = torch.where(some, key >> 32, torch.full_like(key, -1))
            nearest[q] = torch.where(some, key & 0xFFFFFFFF, torch.full_like(key, -1))
            if first_chunk_only:
                return dist2, nearest
    return dist2, nearest


def main():
    scenes = [syn.room_points(s, n_pts=POINTS).astype(np.float32) for s in range(SCENES)]
    offsets = [0]
    for x in scenes:
        offsets.append(offsets[-1] + x.shape[0])
    xyz = torch.from_numpy(np.concatenate(scenes, 0)).to(dev)
    n = xyz.shape[0]
    grid = VoxelGrid(xyz, offsets, voxel_size=VOXEL)
    v = grid.n_voxels
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    pick = torch.rand(n, generator=gen, device=dev)
    common = dict(scenes=SCENES, points=n, voxels=v, voxel_size=VOXEL, window_us=WINDOW_US, chunk=CHUNK)
    for share, reach in CASES:
        sources = pick < share
        held = R._source_voxels(grid, sources, False)
        rows = torch.nonzero(held).reshape(-1)
        src_cells, src_ids = grid.coords[rows].contiguous(), rows.to(torch.int32).contiguous()
        plan = ops.reach_plan(grid.coords, src_cells, src_ids)
        ours = ops.reach_run(plan, reach, err)
        us_kernel, spread, iters = rounds(lambda: ops.reach_run(plan, reach, err))
        us_plan, spread_plan, _ = rounds(lambda: ops.reach_plan(grid.coords, src_cells, src_ids))
        us_call, spread_call, _ = rounds(lambda: R.distance_field(grid, sources, reach))
        ops.reach_check(err)
        torch_field(grid.coords, held, reach, scenes=[0], first_chunk_only=True)
        torch.cuda.synchronize()
        kept, passes = [], []
        for _ in range(TORCH_PASSES):
            passes.append(events_us(lambda: kept.append(torch_field(grid.coords, held, reach)), 1))
        theirs = kept[-1]
        us_torch = statistics.median(passes)
        differing = int(((ours[1].long() != theirs[0]) | (ours[0].long() != theirs[1])).sum())
        emit(kind="field", source_share=share, reach=reach, source_voxels=int(rows.numel()), items=int(plan[2].shape[0]),
             blocks=int(plan[4].shape[0]), found=int((ours[1] >= 0).sum()), us_kernel=us_kernel, us_plan=us_plan, us_call=us_call,
             us_torch=us_torch, torch_over_kernel=us_torch / us_kernel, torch_over_call=us_torch / us_call,
             voxels_differing_between_routes=differing, rounds_us=spread, rounds_plan_us=spread_plan, rounds_call_us=spread_call,
             torch_passes_us=passes, calls_per_window=iters, **common)
        del kept, theirs


if __name__ == "__main__":
    main()
