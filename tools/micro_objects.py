"""Cost of finding objects in heat-maps (csrc/objects.hip) against two yardsticks measured in the same process:

  torch      the same grouping written with what torch offers: thresholding, scatter_reduce(amin) label propagation over
             the same neighbour table until a fixed point (one read-back per sweep), torch.unique, scatter reductions
             and one sort for the ranking (it stops at the sorted records: no [S, Q, M] padding)
  search     ops.bank_search(..., want_heat=True) over a d = 768 bank of the same rows and queries: the pass that produces
             the heat-map the objects are found in

    python tools/micro_objects.py [iters] [out.jsonl]

Two cases: one 150 k-point scene x 1 query, and 8 scenes x 150 k x 32 queries (openscene_amd.synthetic rooms, 5 cm voxels).
The heat-maps are planted clusters (80 % of the hits: the points nearest to four centres per scene and query) plus noise
(20 %: points drawn at random), at hit rates of about 0.1 %, 2 % and 20 % of the points.  HIP events around windows of
about a quarter of a second of back-to-back calls after a warm-up; the variants alternate (A B C A B C A B C) and the
median of the three rounds is reported (rounds_us keeps all of them).  The torch formulation takes seconds per call at
the larger case: it is warmed on one query and then timed over two seconds' worth of calls, or over one call.  One JSON object per line (also appended to out.jsonl when given):
  kind=grid      VoxelGrid construction
  kind=objects   find_objects (us_find; with return_point_ids: us_find_ids), ops.objects_find alone -- no threshold upload,
                 no derived fields -- with the wave-combined atomics (us_ops) and with every hit issuing its own
                 (us_ops_no_combine), the torch formulation (us_torch, sweeps), the search pass (us_search), the two ratios"""
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openscene_amd import ops                                        # noqa: E402
from openscene_amd import synthetic as syn                           # noqa: E402
from openscene_amd.objects import VoxelGrid, find_objects            # noqa: E402

ITERS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
OUT = sys.argv[2] if len(sys.argv) > 2 else None
dev = torch.device("cuda", 0)
VS = 0.05
THR = 0.5
M = 16
ROUNDS = 3


def events_us(f, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def rounds(fs, window_us=250_000.0):
    """us per call of every function of `fs`: a warm-up, then ROUNDS alternating rounds (A B C A B C ...), each timing a
    window of about `window_us` (at most ITERS * 50 calls) between device events; the median of the rounds."""
    iters = []
    for f in fs:
        f()
        f()
        torch.cuda.synchronize()
        est = events_us(f, 3)
        iters.append(max(3, min(ITERS * 50, int(window_us / max(est, 1.0)))))
    got = [[] for _ in fs]
    for _ in range(ROUNDS):
        for i, f in enumerate(fs):
            got[i].append(events_us(f, iters[i]))
    return [statistics.median(g) for g in got], got


def emit(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    if OUT:
        with open(OUT, "a") as fh:
            fh.write(line + "\n")


def planted_heat(xyz, offsets, q_n, rate, gen):
    """fp16 [N, Q]: background below the threshold; per scene and query the 0.8 * rate nearest points to four centres and
    0.2 * rate random points above it."""
    n = xyz.shape[0]
    heat = torch.rand(n, q_n, generator=gen, device=dev) * 0.4
    for a, b in zip(offsets[:-1], offsets[1:]):
        pts = xyz[a:b]
        for j in range(q_n):
            c = pts[torch.randint(0, b - a, (4,), generator=gen, device=dev)]
            dist = torch.cdist(pts, c).min(1)[0]
            k = max(int(0.8 * rate * (b - a)), 1)
            hit = dist <= torch.kthvalue(dist, k)[0]
            hit |= torch.rand(b - a, generator=gen, device=dev) < 0.2 * rate
            col = heat[a:b, j]
            col[hit] = 0.6 + 0.3 * torch.rand(int(hit.sum()), generator=gen, device=dev)
    return heat.half()


BIG = (1 << 62)


def torch_objects(grid, heat, thr, stats=None):
    """The same records with torch only -> (item, peak key, n_points, ...) sorted by (item, peak desc)."""
    n, q_n = heat.shape
    v_n = grid.n_voxels
    inv = grid.inverse.long()
    hf = heat.float()
    hit = torch.isfinite(hf) & (hf >= thr)                                             # [N, Q]
    active = torch.zeros((q_n, v_n), dtype=torch.int32, device=dev)
    active.scatter_reduce_(1, inv[None, :].expand(q_n, -1), hit.t().to(torch.int32), "amax")
    active = active.bool()
    own = torch.arange(v_n, device=dev)[None, :].expand(q_n, -1)
    label = torch.where(active, own, torch.full_like(own, BIG))
    dump = torch.where(grid.nbr >= 0, grid.nbr.long(), torch.full_like(grid.nbr, v_n).long())       # -1 -> a dump column
    ks = [k for k in range(27) if k != 13]
    if grid.connectivity == 6:
        ks = [4, 10, 12, 14, 16, 22]
    sweeps = 0
    while True:
        new = torch.cat([label, torch.full((q_n, 1), BIG, dtype=label.dtype, device=dev)], 1)
        for k in ks:
            new.scatter_reduce_(1, dump[k][None, :].expand(q_n, -1), label, "amin")
        new = torch.where(active, new[:, :v_n], label)
        sweeps += 1
        if torch.equal(new, label):                                                     # (one read-back per sweep)
            break
        label = new
    if stats is not None:
        stats["sweeps"] = sweeps
    p, j = torch.nonzero(hit, as_tuple=True)
    vox = inv[p]
    scene = grid.coords[vox, 0].long()
    key = (scene * q_n + j) * v_n + label[j, vox]
    uniq, comp = torch.unique(key, return_inverse=True)
    c_n = uniq.shape[0]
    score = heat[p, j]
    cnt = torch.bincount(comp, minlength=c_n)
    ssum = torch.zeros(c_n, dtype=torch.int64, device=dev).scatter_add_(0, comp, (score.double() * 2 ** 24).long())
    row = p - grid.offsets_tensor()[scene]
    bits = score.view(torch.int16).long() & 0xFFFF
    skey = torch.where(bits >= 0x8000, 0xFFFF - bits, bits + 0x8000)                    # (finite scores; -0 not folded: a tool)
    peak = torch.zeros(c_n, dtype=torch.int64, device=dev).scatter_reduce_(0, comp, (skey << 32) | (0xFFFFFFFF - row), "amax")
    cells = grid.coords[vox, 1:].long()
    vsum = torch.zeros((c_n, 3), dtype=torch.int64, device=dev).scatter_add_(0, comp[:, None].expand(-1, 3), cells)
    xyz = grid.xyz[p]
    lo = torch.full((c_n, 3), float("inf"), device=dev).scatter_reduce_(0, comp[:, None].expand(-1, 3), xyz, "amin")
    hi = torch.full((c_n, 3), float("-inf"), device=dev).scatter_reduce_(0, comp[:, None].expand(-1, 3), xyz, "amax")
    aq, av = torch.nonzero(active, as_tuple=True)
    vkey = (grid.coords[av, 0].long() * q_n + aq) * v_n + label[aq, av]
    nvox = torch.bincount(torch.searchsorted(uniq, vkey), minlength=c_n)
    item = uniq // v_n
    order = torch.argsort(item * (1 << 48) + ((1 << 48) - 1 - peak))                    # (item, peak desc): the ranking
    return item[order], peak[order], cnt[order], nvox[order], ssum[order], vsum[order], lo[order], hi[order]


def case(scenes, n, q_n, gen):
    rooms = [torch.from_numpy(syn.room_points(s, n_pts=n)) + torch.tensor([6.0 * s, 0.0, 0.0], dtype=torch.float64) for s in range(scenes)]
    xyz = torch.cat(rooms, 0).to(dev)
    offsets = [i * n for i in range(scenes + 1)]
    # the search pass over a d = 768 bank of the same rows and queries, and the grid's construction
    d = 768
    bank = (torch.randn(scenes * n, d, generator=gen, device=dev)).half()
    text = torch.nn.functional.normalize(torch.randn(q_n, d, generator=gen, device=dev), dim=1).half()
    off_dev = torch.tensor(offsets, dtype=torch.int64, device=dev)
    (us_grid, us_search), _ = rounds([lambda: VoxelGrid(xyz, offsets, voxel_size=VS),
                                      lambda: ops.bank_search(bank, off_dev, text, k=16, want_heat=True, max_scene_rows=n)])
    del bank
    grid = VoxelGrid(xyz, offsets, voxel_size=VS)
    emit(kind="grid", scenes=scenes, rows_per_scene=n, voxels=grid.n_voxels, voxel_size=VS, us_grid=us_grid)
    thr = torch.full((q_n,), THR, device=dev)
    for rate in (0.001, 0.02, 0.2):
        heat = planted_heat(grid.xyz, offsets, q_n, rate, gen)
        res = find_objects(grid, heat, THR, max_objects=M)
        hits = int((heat.float() >= THR).sum())
        def kernels(combine):
            return ops.objects_find(heat, thr, grid.xyz, grid.inverse, grid.coords, grid.nbr, grid.offsets_tensor(), max_objects=M,
                                    combine=combine)
        (us_find, us_ids, us_k, us_nc), spread = rounds([
            lambda: find_objects(grid, heat, THR, max_objects=M),
            lambda: find_objects(grid, heat, THR, max_objects=M, return_point_ids=True),
            lambda: kernels(True), lambda: kernels(False)])
        print("# find_objects timed; the torch formulation runs now", flush=True)
        stats = {}
        out = [None]

        def first():
            out[0] = torch_objects(grid, heat, THR, stats)
        torch_objects(grid, heat[:, :1].contiguous(), THR)                     # warm-up on one query: every op's first launch
        us_first = events_us(first, 1)
        assert int(res.n_objects.sum()) == out[0][0].shape[0], (int(res.n_objects.sum()), out[0][0].shape[0])    # same components
        calls = 1
        us_torch = us_first
        if us_first < 2e6:                                                    # (seconds per call otherwise: one call is the measurement)
            calls = max(2, min(20, int(2e6 / us_first)))
            us_torch = events_us(lambda: torch_objects(grid, heat, THR), calls)
        emit(kind="objects", scenes=scenes, rows_per_scene=n, q=q_n, voxels=grid.n_voxels, hit_rate=hits / heat.numel(), hits=hits,
             components=int(res.n_objects.sum()), largest=int(res.n_points.max()), us_find=us_find, us_find_ids=us_ids,
             us_ops=us_k, us_ops_no_combine=us_nc, rounds_us=spread, us_torch=us_torch, torch_calls=calls, torch_sweeps=stats["sweeps"],
             us_search=us_search, torch_over_find=us_torch / us_find, find_over_search=us_find / us_search)


if __name__ == "__main__":
    g = torch.Generator(device=dev).manual_seed(1)
    np.random.seed(0)
    case(1, 150_000, 1, g)
    case(8, 150_000, 32, g)
